"""GPU: point-set neighbours (cgrt_point_grid_*, cgrt_count_point_neighbors*, cgrt_list_point_neighbors*; include/cgrt.h "Point-set
neighbours").  Every case compares bytes three ways: the grid form (the host entries and, through PointGrid, the device
entries), the device brute form, and the numpy restatement (tests/point_neighbors_ref.py, whose own properties
tests/test_point_neighbors_cpu.py holds); counts are compared as well.  m = 4096 data points and n = 2048 queries unless stated.

A full list is kept sorted by insertion in device memory, c^2 / 2 record moves for c neighbours, so the cases in which a query has
thousands of neighbours (r2 = +inf, a radius covering the cloud, far queries that reach in, a cloud of zero extent) compare the k-record
slots with counts and the count call at the full shape, and the full CSR lists at a smaller one.

 1  bucket aliasing: a uniform cloud, cell = radius / 3 (about 7^3 cells per range in 4096 buckets); the work counters show that entries
    of other cells were in fact passed over
 2  the same cloud at six cell sizes, 0.1 x to 100 x the radius (the largest: one cell): the same bytes
 3  r2 = +inf and a radius covering the cloud: the linear walk, says the counter; cell sizes either side of the switch: the same bytes
 4  queries 10 x and 10^6 x the extent outside the box, radii that do and do not reach in; cells visited per query stay within
    (2 ceil(R / h) + 2)^3 and the reaching ones are walked by cells, not linearly: the clamp to cell(hi) works
 5  a self-query with skip_same_index on data with exact duplicates: d2 = 0 ties in index order
 6  per-query radius2 holding NaN, negative, 0 and +inf; r2 = 0 matches coincident points only
 7  non-finite data and queries mixed in; a cloud with no finite point; m = 0; n = 1, 63, 65, 257
 8  coordinates offset by 10^4 with spacing 10^-2, also with a cell far below half extent * 2^-18
 9  a cloud of zero extent
10  the slot rule on the device form: k = 1 .. 9, the full CSR from a count call, a hostile offset table (decreasing pairs, ends beyond
    capacity), canary bytes around d_out
11  one grid queried from two streams and four host threads at once, two of which also build grids of their own meanwhile
12  PointGrid.knn equals the brute k nearest for k = 1, 8, 33 on a uniform and on a clustered cloud (where many queries need three or
    more doublings)
13  data, queries, radius and cell scaled by 2^+-20: the same indices and counts, d2 scaled by 4^+-20 exactly
14  sample_surface_tensor points of a fixture scene: the k = 8 neighbourhoods equal the restatement"""
import math
import threading

import numpy as np
import pytest

import point_neighbors_ref as nref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M, N = 4096, 2048
INF = float("inf")
R = 0.1  # a ball of this radius holds about 17 of 4096 uniform points of the unit cube
R2 = float(np.float32(R * R))
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def sc(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=0)
    yield s
    s.close()


def _uniform(seed, m=M, n=N):
    rng = np.random.default_rng(seed)
    return rng.random((m, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32)


_refs = {}


def _main():
    """The uniform cloud of cases 1, 2, 3, 10, 11: (data, queries, (offsets, records, counts) at R2), computed once, never changed."""
    if "main" not in _refs:
        data, pts = _uniform(7)
        ref = nref.neighbors(pts, data, max_dist2=R2)
        for a in (data, pts, *ref):
            a.setflags(write=False)
        _refs["main"] = (data, pts, ref)
    return _refs["main"]


def _u32(rec):
    """Records of any form as (count, 2) uint32 words."""
    if isinstance(rec, torch.Tensor):
        rec = rec.cpu().numpy()
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 2)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _same(got, want, what):
    got, want = _u32(got), _u32(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} records differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _check(sc, data, pts, cell, radius2=None, max_dist2=INF, skip=False, k=5, full=True, ref=None, host=True, brute=True):
    """All forms against the restatement: counts, k-record slots with and without counts, and (full) the CSR lists.  Returns the
    restatement's (offsets, records, counts)."""
    off_r, rec_r, cnt_r = ref if ref is not None else nref.neighbors(pts, data, radius2, max_dist2, skip)
    slots_r = nref.first_k(off_r, rec_r, k)
    kw = dict(radius2=radius2, max_dist2=max_dist2, skip_same_index=skip)
    n = len(pts)
    if host:
        assert np.array_equal(sc.count_point_neighbors(data, cell, pts, **kw), cnt_r), "host count"
        rec, cnt = sc.nearest_points(data, cell, pts, k, want_counts=True, **kw)
        _same(rec, slots_r, "host slots with counts")
        assert np.array_equal(cnt, cnt_r)
        _same(sc.nearest_points(data, cell, pts, k, **kw), slots_r, "host slots")
        if full:
            off, rec = sc.list_point_neighbors(data, cell, pts, **kw)
            assert np.array_equal(off, off_r)
            _same(rec, rec_r, "host lists")
    if brute:
        rec, cnt = sc.list_point_neighbors_brute(data, pts, k=k, **kw)
        _same(rec, slots_r, "brute slots")
        assert np.array_equal(cnt, cnt_r), "brute counts"
        if full:
            off, rec = sc.list_point_neighbors_brute(data, pts, **kw)
            assert np.array_equal(off, off_r)
            _same(rec, rec_r, "brute lists")
    grid = sc.point_grid_tensor(_t(data), cell)
    tp = _t(pts)
    tkw = dict(radius2=None if radius2 is None else _t(np.asarray(radius2, np.float32)), max_dist2=max_dist2, skip_same_index=skip)
    assert np.array_equal(grid.count(tp, **tkw).cpu().numpy().view(np.uint32), cnt_r), "device count"
    rec, cnt = grid.nearest(tp, k, want_counts=True, **tkw)
    _same(rec, slots_r, "device slots with counts")
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), cnt_r)
    _same(grid.nearest(tp, k, **tkw), slots_r, "device slots")
    if full:
        off, rec = grid.list(tp, **tkw)
        assert np.array_equal(off.cpu().numpy(), off_r) and n == len(off_r) - 1
        _same(rec, rec_r, "device lists")
    return off_r, rec_r, cnt_r


# ---- 1, 2, 3 ----
def test_bucket_aliasing(sc):
    data, pts, ref = _main()
    cell = R / 3
    _check(sc, data, pts, cell, max_dist2=R2, ref=ref)
    w = sc.debug_point_neighbor_work(data, cell, pts, max_dist2=R2)
    print("work:", w)
    assert w["foreign"] > 0, "no entry of another cell was met: the case shows nothing"
    assert w["linear"] == 0 and w["entries"] - w["foreign"] == w["d2_evals"] and 0 < w["buckets_used"] <= 4096
    assert w["cells"] <= N * 8**3 and ref[2].sum() <= w["d2_evals"]


@pytest.mark.parametrize("factor", [0.1, 0.3, 1.0, 3.0, 10.0, 100.0])
def test_cell_sizes(sc, factor):
    data, pts, ref = _main()
    _check(sc, data, pts, R * factor, max_dist2=R2, ref=ref, brute=False)
    if factor == 100.0:
        w = sc.debug_point_neighbor_work(data, R * factor, pts, max_dist2=R2)
        assert w["buckets_used"] == 1 and w["cells"] == N and w["foreign"] == 0 and w["d2_evals"] == N * M, "everything in one cell"


def test_linear_walk(sc):
    data, pts, _ = _main()
    ref, cell = None, R / 2  # (20 cells per axis over the cloud, 8000 in all: more than the 4096 entries)
    for r2 in (INF, 4.0):  # (the unit cube's diagonal squared is 3: both bounds hold the whole cloud, in the same order)
        ref = _check(sc, data, pts, cell, max_dist2=r2, full=False, ref=ref)
        assert (ref[2] == M).all()
        for k in (0, 5):
            w = sc.debug_point_neighbor_work(data, cell, pts, max_dist2=r2, k=k)
            assert w["linear"] == N and w["cells"] == 0 and w["foreign"] == 0 and w["entries"] == N * M == w["d2_evals"], (r2, k, w)
    d, p = data[:512], pts[:257]
    _check(sc, d, p, R, max_dist2=INF)
    _check(sc, d, p, R, max_dist2=4.0, skip=True)


def test_either_side_of_the_switch(sc):
    """A range of up to 16 cells per axis has at most 4096 cells, not more than the entries: walked by cells; from 18 per axis on it has
    more: the entry array is walked (queries near the box's faces have clamped, smaller ranges)."""
    data, pts, ref = _main()
    coarse, fine = 2 * R / 14, 2 * R / 17
    lin = []
    for cell in (coarse, fine):
        _check(sc, data, pts, cell, max_dist2=R2, ref=ref, brute=False, host=False)
        lin.append(sc.debug_point_neighbor_work(data, cell, pts, max_dist2=R2)["linear"])
    print("queries on the linear walk either side of the switch:", lin)
    assert lin[0] == 0 and 0 < lin[1] < N


# ---- 4 ----
@pytest.mark.parametrize("far", [10.0, 1e6])
def test_queries_outside_the_box(sc, far):
    data, _, _ = _main()
    rng = np.random.default_rng(11)
    n = 256
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (0.5 + d * far).astype(np.float32)
    dist = np.linalg.norm(pts.astype(np.float64) - 0.5, axis=1)
    cell = 0.1
    reach = np.where(np.arange(n) % 2 == 0, dist + 0.3, dist - 3.0).astype(np.float32)  # (the cube lies within 0.87 of its centre)
    r2 = (reach * reach).astype(np.float32)
    ref = _check(sc, data, pts, cell, radius2=r2, k=8, full=False)
    assert (ref[2][1::2] == 0).all() and (ref[2][0::2] > 0).all(), "every second radius reaches in"
    for part, name in ((slice(0, None, 2), "reach"), (slice(1, None, 2), "miss")):
        w = sc.debug_point_neighbor_work(data, cell, pts[part], radius2=r2[part])
        bound = sum((2 * math.ceil(float(x) / cell) + 2) ** 3 for x in reach[part])
        print(far, name, w)
        assert w["cells"] <= bound
        assert w["cells"] <= (n // 2) * 11**3 and w["linear"] == 0, "the range is clamped to the data's cells, and walked by cells"


# ---- 5, 6 ----
def test_self_query_with_duplicates(sc):
    rng = np.random.default_rng(5)
    base = rng.random((512, 3)).astype(np.float32)
    data = base[rng.integers(0, 512, 2048)]  # about four copies of each
    off, rec, cnt = _check(sc, data, data, R, max_dist2=R2, skip=True)
    first = rec[off[:-1][cnt > 0]]
    assert (first["dist2"] == 0).sum() > 1500, "most points have a coincident copy"
    for i in (0, 1, 2, 100):
        zero = rec[off[i] : off[i + 1]]
        zero = zero[zero["dist2"] == 0]["index"]
        assert (np.diff(zero.astype(np.int64)) > 0).all() and i not in zero
    _check(sc, data, data, R, max_dist2=R2, skip=False, brute=False)


def test_per_query_radii(sc):
    data, _, _ = _main()
    pts = data[:N].copy()
    r2 = np.full(N, R2, np.float32)
    r2[0::8], r2[1::8], r2[2::8] = np.nan, -1.0, 0.0
    r2[3::64] = np.inf
    r2[4::8] = -np.inf
    r2[5::8] = -0.0
    off, rec, cnt = _check(sc, data, pts, R, radius2=r2, k=8, full=False)
    assert (cnt[0::8] == 0).all() and (cnt[1::8] == 0).all() and (cnt[4::8] == 0).all() and (cnt[3::64] == M).all()
    assert (cnt[2::8] == 1).all() and (cnt[5::8] == 1).all(), "r2 = 0: the coincident point alone"
    _check(sc, data, pts, R, radius2=r2, k=8, full=False, skip=True, brute=False)
    finite = np.where(np.isposinf(r2), np.float32(R2), r2)
    _check(sc, data, pts, R, radius2=finite)


# ---- 7 ----
def test_non_finite_points(sc):
    rng = np.random.default_rng(3)
    data, pts = _uniform(3)
    bad = np.asarray([np.nan, np.inf, -np.inf], np.float32)
    for a, count in ((data, 300), (pts, 200)):
        idx = rng.choice(len(a), count, replace=False)
        a[idx, rng.integers(0, 3, count)] = rng.choice(bad, count)
    off, rec, cnt = _check(sc, data, pts, R, max_dist2=R2)
    assert (cnt[~nref.finite(pts)] == 0).all() and nref.finite(data)[rec["index"]].all()
    ref = _check(sc, data, pts, R, max_dist2=INF, k=8, full=False)
    assert set(np.unique(ref[2])) == {0, int(nref.finite(data).sum())}


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_lengths_and_empty_clouds(sc, n):
    data, pts = _uniform(100 + n, m=777, n=n)
    _check(sc, data, pts, 2 * R, max_dist2=np.float32(4 * R2))
    nothing = np.full((64, 3), np.nan, np.float32)
    nothing[::2, 1] = np.inf
    for d in (nothing, np.zeros((0, 3), np.float32)):
        for r2 in (R2, INF):
            ref = _check(sc, d, pts, R, max_dist2=r2)
            assert ref[2].sum() == 0


# ---- 8, 9 ----
def test_offset_coordinates(sc):
    rng = np.random.default_rng(8)
    g = np.arange(16, dtype=np.float64) * 1e-2
    data = (1e4 + np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)).astype(np.float32)
    pts = (1e4 + rng.random((N, 3)) * 0.15).astype(np.float32)
    pts[:512] = data[rng.integers(0, len(data), 512)]
    r2 = np.float32(0.015**2)
    ref = _check(sc, data, pts, 0.015, max_dist2=r2)
    assert 3 < ref[2].mean() < 40
    # a cell far below half extent * 2^-18 (about 3e-7 here): the rule sets the edge; the range of r2 then has more cells than entries
    _check(sc, data, pts, 1e-12, max_dist2=r2, ref=ref, brute=False)
    w = sc.debug_point_neighbor_work(data, 1e-12, pts, max_dist2=r2)
    assert w["linear"] == N
    # ... and r2 = 0 is a walk over a few cells of that edge, which finds the coincident points
    zero = _check(sc, data, pts, 1e-12, max_dist2=0.0, brute=False)
    assert (zero[2][:512] >= 1).all()
    w = sc.debug_point_neighbor_work(data, 1e-12, pts, max_dist2=0.0)
    assert w["linear"] == 0 and 0 < w["cells"] <= 27 * N


def test_zero_extent(sc):
    _, pts, _ = _main()
    one = np.float32([0.25, 0.5, 0.75])
    pts = pts.copy()
    pts[::16] = one
    data = np.tile(one, (M, 1))
    ref = _check(sc, data, pts, R, max_dist2=R2, k=8, full=False)
    assert set(np.unique(ref[2])) == {0, M} and (ref[2][::16] == M).all()
    _check(sc, data[:100], pts[:300], R, max_dist2=R2)
    _check(sc, data[:100], pts[:300], R, max_dist2=0.0, brute=False)


# ---- 10 ----
class Guarded:
    """`records` 8-byte records of device memory between two guards, every byte SENTINEL before the call."""

    PAD = 256

    def __init__(self, records):
        self.n = int(records) * 8
        self.buf = torch.full((self.n + 2 * self.PAD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.buf.data_ptr() + self.PAD

    def words(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[self.PAD : self.PAD + self.n].view(np.uint32).reshape(-1, 2)

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[: self.PAD] == SENTINEL).all() and (b[self.PAD + self.n :] == SENTINEL).all())


@pytest.mark.parametrize("k", range(1, 10))
def test_device_slots_of_k_records(sc, k):
    data, pts, ref = _main()
    grid = sc.point_grid_tensor(_t(data), R)
    tp = _t(pts)
    want = nref.first_k(ref[0], ref[1], k)
    for counted in (False, True):
        out, cnt = Guarded(N * k), torch.full((N,), 77, dtype=torch.int32, device="cuda")
        sc.list_point_neighbors_device(grid.grid.data_ptr(), grid.grid.numel(), tp.data_ptr(), N, out.ptr(), N * k, k=k,
                                       d_counts_ptr=cnt.data_ptr() if counted else 0, max_dist2=R2)
        _same(out.words(), want, f"k = {k}")
        assert out.intact()
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), ref[2]) if counted else (cnt == 77).all()


def test_device_csr_and_hostile_offsets(sc):
    data, pts, ref = _main()
    off_r, rec_r, cnt_r = ref
    grid = sc.point_grid_tensor(_t(data), R)
    g, gb = grid.grid.data_ptr(), grid.grid.numel()
    tp = _t(pts)
    off, rec = grid.list(tp, max_dist2=R2)  # the full CSR from a count call
    assert np.array_equal(off.cpu().numpy(), off_r)
    _same(rec, rec_r, "CSR")
    # a hostile table: the true offsets up to query 1000, whose slots a capacity in the middle of query 900 truncates and empties;
    # then decreasing pairs and ends beyond the capacity; queries 0 .. 3 own overlapping slots but have no neighbours (radius -1), so
    # whichever of them writes last, the bytes are the same
    cap = int(off_r[900]) + 3
    hostile = off_r.astype(np.uint64).copy()
    a = int(off_r[4])
    assert a >= 2
    hostile[0:4] = [a, 1, a // 2, 0]  # slots [a, 1) -> empty, [1, a / 2), [a / 2, 0) -> empty, [0, a): all padding, inside query 3's
    hostile[1001:] = np.resize(np.asarray([cap + 100, cap + 50, 2**63, cap, 2**64 - 1, cap + 7], np.uint64), N - 1000)
    hostile[N] = 0
    r2 = np.full(N, R2, np.float32)
    r2[:4] = -1.0
    r2[1000:] = -1.0
    want = np.full((cap, 2), SENTINEL * 0x01010101, np.uint32)
    mine = nref.neighbors(pts, data, radius2=r2)
    for i in range(N):
        b, e = int(hostile[i]), int(hostile[i + 1])
        b, e = min(b, cap), min(max(e, b), cap)
        have = _u32(mine[1][mine[0][i] : mine[0][i + 1]])[: e - b]
        want[b : b + len(have)] = have
        want[b + len(have) : e] = [0x7F800000, 0xFFFFFFFF]
    out, cnt = Guarded(cap), torch.zeros((N,), dtype=torch.int32, device="cuda")
    sc.list_point_neighbors_device(g, gb, tp.data_ptr(), N, out.ptr(), cap, d_offsets_ptr=_t(hostile.view(np.int64)).data_ptr(),
                                   d_counts_ptr=cnt.data_ptr(), d_radius2_ptr=_t(r2).data_ptr())
    got = out.words()
    assert out.intact(), "a record was written outside the first `capacity` records"
    _same(got, want, "hostile offsets")
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), mine[2]), "the counts are the full counts whatever the slots hold"
    assert (got[int(off_r[4]) : int(off_r[900])] == _u32(rec_r[off_r[4] : off_r[900]])).all() and mine[2][4:1000].sum() > 0


# ---- 11 ----
def test_two_streams_and_four_threads(sc):
    data, pts, ref = _main()
    off_r, rec_r, cnt_r = ref
    want = nref.first_k(off_r, rec_r, 6)
    td, tp = _t(data), _t(pts)
    shared = sc.point_grid_tensor(td, R)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    results, errors = [None] * 4, []

    def work(t):
        try:
            s = streams[t]
            with torch.cuda.stream(s):
                grid = shared if t < 2 else sc.point_grid_tensor(td, R * (t - 1), stream=s)  # (2, 3: builds of their own, meanwhile)
                dev = []
                for _ in range(3):
                    dev.append((grid.nearest(tp, 6, max_dist2=R2, stream=s), grid.count(tp, max_dist2=R2, stream=s)))
                s.synchronize()
            host = sc.nearest_points(data, R * (t + 1), pts, 6, max_dist2=R2, want_counts=True)
            results[t] = (dev, host)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for dev, host in results:
        for rec, cnt in dev:
            _same(rec, want, "device, threaded")
            assert np.array_equal(cnt.cpu().numpy().view(np.uint32), cnt_r)
        _same(host[0], want, "host, threaded")
        assert np.array_equal(host[1], cnt_r)


# ---- 12 ----
def _clustered(seed):
    rng = np.random.default_rng(seed)
    centres = rng.random((64, 3))
    data = (centres[rng.integers(0, 64, M)] + rng.normal(size=(M, 3)) * 1e-3).astype(np.float32)
    return data, rng.random((N, 3)).astype(np.float32)


@pytest.mark.parametrize("cloud", ["uniform", "clustered"])
def test_knn_equals_the_brute_k_nearest(sc, cloud):
    data, pts = _uniform(12) if cloud == "uniform" else _clustered(12)
    cell = 0.05 if cloud == "uniform" else 0.01
    grid = sc.point_grid_tensor(_t(data), cell)
    tp = _t(pts)
    if cloud == "clustered":
        c8 = sc.count_point_neighbors(data, cell, pts, max_dist2=np.float32((8 * cell) ** 2))
        print("queries with fewer than 33 points within 8 cells:", int((c8 < 33).sum()))
        assert (c8 < 33).sum() > N // 4, "many queries need more than three doublings"
    for k in (1, 8, 33):
        want, _ = sc.list_point_neighbors_brute(data, pts, k=k)
        _same(grid.knn(tp, k), want, f"knn, k = {k}")
    small, _ = sc.list_point_neighbors_brute(data[:20], data[:20], k=33, skip_same_index=True)
    g20 = sc.point_grid_tensor(_t(data[:20]), cell)
    _same(g20.knn(_t(data[:20]), 33, skip_same_index=True), small, "fewer than k data points")
    assert (small["index"][:, 19:] == nref.NO_PRIM).all() and (small["index"][:, :19] != np.arange(20)[:, None]).all()
    self_want, _ = sc.list_point_neighbors_brute(data[:N], data[:N], k=8, skip_same_index=True)
    _same(sc.point_grid_tensor(_t(data[:N]), cell).knn(_t(data[:N]), 8, skip_same_index=True), self_want, "self knn")


# ---- 13, 14 ----
@pytest.mark.parametrize("e", [-20, 20])
def test_scaling_by_a_power_of_two(sc, e):
    data, pts, ref = _main()
    s = np.float32(2.0**e)
    off, rec, cnt = _check(sc, data * s, pts * s, R * float(s), max_dist2=np.float32(R2) * s * s, brute=False)
    assert np.array_equal(cnt, ref[2]) and np.array_equal(off, ref[0]) and np.array_equal(rec["index"], ref[1]["index"])
    assert np.array_equal(rec["dist2"], ref[1]["dist2"] * (s * s)), "d2 scales by 4^e exactly"


def test_surface_samples_of_a_fixture_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("monkey"), device=0)
    try:
        p = s.sample_surface_tensor(N, seed=14)["point"].contiguous()
        data = p.cpu().numpy()
        area = s.triangle_areas()[1]
        r = math.sqrt(16 * area / (math.pi * N))  # a disk of this radius on the surface holds about 16 of the samples
        r2 = float(np.float32(r * r))
        grid = s.point_grid_tensor(p, r)
        rec, cnt = grid.nearest(p, 8, max_dist2=r2, skip_same_index=True, want_counts=True)
        want, wc = nref.neighbors(data, data, max_dist2=r2, skip_same_index=True, k=8)
        _same(rec, want, "k = 8 neighbourhoods of surface samples")
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), wc) and 4 < wc.mean() < 64
        _same(grid.knn(p, 8, skip_same_index=True), s.list_point_neighbors_brute(data, data, k=8, skip_same_index=True)[0], "knn")
    finally:
        s.close()

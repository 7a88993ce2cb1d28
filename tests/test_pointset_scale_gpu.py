"""GPU: point-set neighbours and Poisson-disk sets across scale and past 2^18 buckets (include/cgrt.h "Point-set neighbours" and
"Poisson-disk sets", their "Envelope" paragraphs).  The helpers are held by tests/test_pointset_scale_cpu.py.

* Neighbours at EVERY scale 2^k, k in KS and 100, inside the envelope or not: point_neighbors_ref.scale_cloud() (4 096 data points, 2 048
  queries) with data, queries and cell multiplied by 2^k (np.ldexp); bounds +inf, FLT_MAX, r2 * 2^2k (0.0 where it underflows) and a
  per-query array cycling through 0.0, -0.0, a subnormal, r2 * 2^2k, +inf, NaN and -1.  Grid form (host entries and PointGrid) ==
  device brute form == restatement by bytes: counts, k = 8 slots with and without counts, full CSR lists (on 256 data points and 300
  queries where the mean count exceeds 64).  Reached, and asserted: subnormal d2 in the lists at 2^-70; every count 4 096 at 2^-80 under
  r2 = 0, walked by cells; +inf d2 at 2^64 that qualifies under +inf only and ties by ascending index; a subnormal cell.
* Covariance at k in (-31, -20, 30, 62), where every query is inside: the device's lists are the image of the device's lists at scale 1
  and debug_point_neighbor_work equals its values at scale 1.
* A cloud at +-2^127 u, whose `x - lo` overflows (cell() clamps at 2^21 - 1), and the same at 2^126: bounds +inf, FLT_MAX and 0, three
  forms by bytes; under 0 a coincident query finds exactly its duplicates.
* 266 241 data points (2^19 buckets: the shared scan's carry loop runs twice), 1 % of them NaN, 257 queries: grid == brute ==
  restatement; under +inf every count is the number of finite data points (the grand total behind the last bucket).
* Poisson at 2^e, e in (-75, -70, -62, 62, 64), min_dist2 times 2^2e, on 4 097 monkey samples: host == device == brute == restatement;
  the flags of scale 1 where min_dist2 stays normal; every point kept at 2^-75.  The overflowing cloud with min_dist2 1.0 and FLT_MAX: a
  d2 of +inf is never a conflict.
* Poisson on 270 000 uniform points (2^19 buckets): the device form == poisson_ref.greedy_sparse."""
import numpy as np
import pytest

import point_neighbors_ref as nref
import poisson_ref as pref
import scale_ref as sref
from test_point_neighbors_gpu import M, N, _check, _same, _t, sc  # noqa: F401  (sc: fixture)
from test_poisson_gpu import _device, _form, _reference, scenes  # noqa: F401  (scenes: fixture)
from test_poisson_gpu import _same as _same_flags

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
KS = (-80, -70, -45, -31, -20, 0, 30, 62, 64)
ALL_KS = KS + (100,)
INSIDE_KS = (-31, -20, 30, 62)
INF = float("inf")
FLT_MAX, FLT_MIN = sref.FLT_MAX, sref.FLT_MIN
CELL = F32(0.1)
R2 = float(F32(0.1) * F32(0.1))
SMALL = (256, 300)  # data points and queries of the full lists where a query has thousands of neighbours
LABELS = ("+inf", "FLT_MAX", "radius", "per query")

_cache = {}


def _r2(k):
    with np.errstate(all="ignore"):
        return F32(np.ldexp(F32(R2), 2 * int(k)))


def _cell(k):
    """the cell edge times 2^k, replaced by the smallest normal float or by 2^126 where that would be 0 or +inf"""
    with np.errstate(all="ignore"):
        c = F32(np.ldexp(CELL, int(k)))
    return float(FLT_MIN if c == 0 else 2.0 ** 126 if np.isinf(c) else c)


def _cloud(k):
    if "cloud" not in _cache:
        _cache["cloud"] = nref.scale_cloud()
        assert _cache["cloud"][0].shape == (M, 3) and _cache["cloud"][1].shape == (N, 3)
    data, pts = _cache["cloud"]
    return sref.scaled_points(data, k), sref.scaled_points(pts, k)


def _bound(k, label):
    """(radius2 array or None, max_dist2)"""
    rk = _r2(k)
    if label == "+inf":
        return None, INF
    if label == "FLT_MAX":
        return None, FLT_MAX
    if label == "radius":
        assert np.isfinite(rk)
        return None, float(rk)  # (0.0 where r2 * 2^2k underflows)
    cycle = np.array([0.0, -0.0, 1e-42, rk, np.inf, np.nan, -1.0], F32)
    assert np.signbit(cycle[1]) and 0 < cycle[2] < FLT_MIN
    return np.ascontiguousarray(cycle[np.arange(N) % len(cycle)]), INF


CASES = [(k, label) for k in ALL_KS for label in LABELS if not (label == "radius" and np.isinf(_r2(k)))]


def _records(off, rec):
    return off.cpu().numpy(), np.ascontiguousarray(rec.cpu().numpy()).view(nref.RECORD).reshape(-1)


# ---- neighbours across scale ----
@pytest.mark.parametrize("k, label", CASES, ids=[f"2^{k} {label}" for k, label in CASES])
def test_neighbours_at_every_scale(sc, k, label):
    data, pts = _cloud(k)
    assert np.isfinite(data).all() and np.isfinite(pts).all()
    cell = _cell(k)
    radius2, md = _bound(k, label)
    off, rec, cnt = nref.neighbors(pts, data, radius2, md)
    many = cnt.mean() > 64
    print(f"2^{k}, {label}: cell {cell:g}, mean count {cnt.mean():.1f}")
    _check(sc, data, pts, cell, radius2=radius2, max_dist2=md, k=8, full=not many, ref=(off, rec, cnt))
    if many:
        d, p = data[: SMALL[0]], pts[: SMALL[1]]
        _check(sc, d, p, cell, radius2=None if radius2 is None else radius2[: SMALL[1]], max_dist2=md, k=8)
    d2 = rec["dist2"]
    if k == -70 and label == "radius":
        assert 0 < md < FLT_MIN and ((d2 > 0) & (d2 < FLT_MIN)).sum() > 1000, "subnormal d2 in the lists at 2^-70"
    if k == -80 and label == "radius":
        assert md == 0.0 and (cnt == M).all() and (d2 == 0).all(), "every d2 underflows to 0 at 2^-80"
        w = sc.debug_point_neighbor_work(data, cell, pts, max_dist2=0.0)
        print("work:", w)
        assert w["linear"] == 0 and 0 < w["cells"] <= N * 11 ** 3 and w["d2_evals"] == N * M, "the reach of r2 = 0 covers the cloud, by cells"
        tiny = 1e-40  # a subnormal cell: the rule h = max(cell, half extent * 2^-18) sets the edge
        assert 0 < F32(tiny) < FLT_MIN
        _check(sc, data, pts, tiny, max_dist2=0.0, k=8, full=False, ref=(off, rec, cnt), brute=False)
    if k == 64 and label in ("+inf", "FLT_MAX"):
        finite_d2 = (nref.d2_matrix(pts, data) <= F32(FLT_MAX)).sum(1)
        assert (finite_d2 < M).sum() > N // 2 and finite_d2.sum() > 0, "most queries have a data point more than 2^64 away"
        if label == "FLT_MAX":
            assert np.array_equal(cnt, finite_d2) and np.isfinite(d2).all(), "+inf d2 qualifies under +inf only"
        else:
            assert (cnt == M).all() and np.isposinf(d2).sum() == N * M - finite_d2.sum()
            for i in np.argsort(finite_d2, kind="stable")[:3]:
                tail = rec[off[i] : off[i + 1]][finite_d2[i] :]
                assert np.isposinf(tail["dist2"]).all() and (np.diff(tail["index"].astype(np.int64)) > 0).all(), "ties by ascending index"


def _device_lists(sc, k):
    if ("lists", k) not in _cache:
        data, pts = _cloud(k)
        grid = sc.point_grid_tensor(_t(data), _cell(k))
        _cache[("lists", k)] = (_records(*grid.list(_t(pts), max_dist2=float(_r2(k)))),
                                [sc.debug_point_neighbor_work(data, _cell(k), pts, max_dist2=float(_r2(k)), k=kk) for kk in (0, 8)])
    return _cache[("lists", k)]


@pytest.mark.parametrize("k", INSIDE_KS)
def test_neighbour_lists_are_covariant_inside_the_envelope(sc, k):
    data, pts = _cloud(0)
    inside = sref.in_point_envelope(sref.point_measures(pts, data), R2, k)
    assert inside.all(), "every query is inside at this scale"
    (full0, work0), (fullk, workk) = _device_lists(sc, 0), _device_lists(sc, k)
    assert len(full0[1]) > 10 * N
    cov = sref.covariant_point_neighbors(full0, fullk, k)
    assert cov.all(), (k, int((~cov).sum()), int(np.flatnonzero(~cov)[0]))
    assert workk == work0, (k, workk, work0)


# ---- a cloud whose extent overflows ----
@pytest.mark.parametrize("k", [127, 126])
@pytest.mark.parametrize("label", ["+inf", "FLT_MAX", "0"])
def test_a_cloud_whose_extent_overflows(sc, k, label):
    data, pts = nref.overflow_cloud(k)
    lo = data.min(0)
    with np.errstate(over="ignore"):
        assert np.isposinf(data - lo).any() == (k == 127), "x - lo overflows for part of the cloud at 2^127 only"
    md = {"+inf": INF, "FLT_MAX": FLT_MAX, "0": 0.0}[label]
    cell = 2.0 ** (k - 7)
    if label == "+inf":
        ref = _check(sc, data, pts, cell, max_dist2=md, k=8, full=False)
        assert (ref[2] == len(data)).all() and np.isposinf(ref[1]["dist2"]).sum() > len(pts) * (len(data) - 8)
        _check(sc, data[: SMALL[0]], pts[: SMALL[1]], cell, max_dist2=md, k=8)
        return
    off, rec, cnt = _check(sc, data, pts, cell, max_dist2=md, k=8)
    dup = (pts[:, None, :] == data[None, :, :]).all(2).sum(1)
    assert (dup[0:256:2] == 2).all() and (dup[256::2] == 1).all() and (dup[1::2] == 0).all()
    assert np.array_equal(cnt, dup) and (rec["dist2"] == 0).all(), "exactly the duplicates: every other d2 is +inf"
    if label == "0":
        w = sc.debug_point_neighbor_work(data, cell, pts, max_dist2=0.0)
        assert w["linear"] == 0 and 0 < w["cells"] <= 27 * len(pts), w


# ---- past 2^18 buckets ----
BIG_M = 262_145 + 4096


def test_neighbours_past_2_18_buckets(sc):
    rng = np.random.default_rng(41)
    data = rng.random((BIG_M, 3)).astype(F32)
    bad = rng.choice(BIG_M, BIG_M // 100, replace=False)
    data[bad, rng.integers(0, 3, len(bad))] = np.nan
    pts = rng.random((257, 3)).astype(F32)
    pts[::4] = data[np.flatnonzero(nref.finite(data))[:65]]
    buckets = (sc.point_grid_workspace(BIG_M) - 24 * BIG_M) // 8
    assert 1 << 19 <= buckets < (1 << 19) + 1024, "2^19 buckets are 512 scan tiles: the carry loop runs twice"
    r = (16.0 / (4.0 / 3.0 * np.pi * BIG_M)) ** (1.0 / 3.0)  # a ball of this radius holds about 16 of the points
    r2 = float(F32(r * r))
    used = sc.debug_point_neighbor_work(data, r, pts[:1], max_dist2=0.0)["buckets_used"]
    assert used > 1 << 15, ("41^3 cells hashed over 512 tiles: the 256 of the second pass are populated", used)
    off, rec, cnt = nref.neighbors(pts, data, max_dist2=r2, block=64)
    assert 8 < cnt.mean() < 32 and nref.finite(data)[rec["index"]].all()
    want = nref.first_k(off, rec, 8)
    td, tp = _t(data), _t(pts)
    grid = sc.point_grid_tensor(td, r)
    got, gc = grid.nearest(tp, 8, max_dist2=r2, want_counts=True)
    _same(got, want, "grid slots")
    assert np.array_equal(gc.cpu().numpy().view(np.uint32), cnt), "grid counts"
    assert np.array_equal(grid.count(tp, max_dist2=r2).cpu().numpy().view(np.uint32), cnt), "grid count call"
    goff, grec = grid.list(tp, max_dist2=r2)
    assert np.array_equal(goff.cpu().numpy(), off)
    _same(grec, rec, "grid lists")
    brec, bcnt = sc.list_point_neighbors_brute(data, pts, k=8, max_dist2=r2)
    _same(brec, want, "brute slots")
    assert np.array_equal(bcnt, cnt), "brute counts"
    # r2 = +inf: the linear walk reads the number of entries from the scan's grand total
    nfin = int(nref.finite(data).sum())
    assert nfin == BIG_M - len(bad)
    assert (grid.count(tp).cpu().numpy() == nfin).all(), "every finite data point, once"
    irec, icnt = grid.nearest(tp, 8, want_counts=True)
    brec, bcnt = sc.list_point_neighbors_brute(data, pts, k=8)
    _same(irec, brec, "k = 8 nearest under +inf")
    assert np.array_equal(icnt.cpu().numpy().view(np.uint32), bcnt) and (bcnt == nfin).all()
    _same(irec.cpu().numpy()[cnt >= 8], want[cnt >= 8], "the 8 nearest within r2 are the 8 nearest")


# ---- Poisson across scale ----
@pytest.mark.parametrize("e", [-75, -70, -62, 62, 64])
def test_poisson_at_every_scale(scenes, e):
    p, res = _reference(scenes, "monkey", 4097, 1)
    _, sc_, _ = scenes("monkey")
    m, want = res[10]
    ps = sref.scaled_points(p, e)
    with np.errstate(all="ignore"):
        ms = F32(np.ldexp(F32(m), 2 * e))
    assert np.isfinite(ps).all() and np.isfinite(ms)
    ref = pref.greedy(ps, ms, seed=1)
    for form in ("host", "device", "brute"):
        _same_flags(_form(sc_, form, ps, ms, seed=1), ref, (form, e))
    print(f"2^{e}: min_dist2 {ms:g}, {int(ref.sum())} kept ({int(want.sum())} at scale 1)")
    assert (ms >= FLT_MIN) == (e > 0)
    if ms >= FLT_MIN:
        assert np.array_equal(ref, want), "the flags of scale 1 while min_dist2 stays normal"
    if e == -75:
        assert ms == 0 and ref.all(), "min_dist2 underflows to 0: every finite point is kept"
    if e == -70:
        assert 0 < ms < 64 * 1.4e-45, "min_dist2 is a few subnormal ulps"


@pytest.mark.parametrize("m", [1.0, FLT_MAX])
def test_poisson_on_the_overflowing_cloud(scenes, m):
    _, sc_, _ = scenes("cube")
    p = nref.overflow_cloud(127)[0]
    ref = pref.greedy(p, m, seed=6)
    assert (ref[:64] ^ ref[64:128]).all() and ref[128:].all(), "only exact duplicates conflict, one of each pair is kept: +inf never conflicts"
    for form in ("host", "device", "brute"):
        _same_flags(_form(sc_, form, p, m, seed=6), ref, (form, m))


# ---- Poisson past 2^18 buckets ----
def test_poisson_past_2_18_buckets(scenes):
    _, sc_, _ = scenes("cube")
    n = 270_000
    p = np.random.default_rng(43).random((n, 3)).astype(F32)
    r = (8.0 / (4.0 / 3.0 * np.pi * n)) ** (1.0 / 3.0)  # a ball of this radius holds about 8 of the points
    m = F32(r * r)
    pairs = pref.conflict_pairs(p, m)
    assert 4 < 2 * len(pairs) / n < 12, "about 8 conflicts per point"
    want = pref.greedy_sparse(p, m, seed=9, pairs=pairs)
    got = _device(sc_, p, m, seed=9)
    _same_flags(got, want, "device form, 270 000 points")
    assert n / 32 <= got.sum() < n
    w = sc_.debug_poisson_work(p, float(m), seed=9)
    # (about 52^3 cells of edge R, most of them occupied, hashed over 2^19 buckets: some 10^5 in use, 200 per tile)
    assert w["buckets"] == 1 << 19 and w["buckets_used"] > 1 << 15, ("512 scan tiles, those of the second pass populated", w)
    sub = np.flatnonzero(got)[:4096]
    assert not pref.conflicts(p[sub], m).any(), "kept points do not conflict (the first 4 096 of them, all pairs)"
    # maximal: every point that is not kept conflicts with a kept point before it
    key = pref.keys(n, 9)
    a, b = pairs[:, 0], pairs[:, 1]
    covered = np.zeros(n, bool)
    covered[a[got[b] & (key[b] < key[a])]] = True
    covered[b[got[a] & (key[a] < key[b])]] = True
    assert (covered | got).all() and not (got[a] & got[b]).any()

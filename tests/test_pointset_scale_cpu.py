"""No GPU: the helpers of the point-set tests across scale and at size (tests/test_pointset_scale_gpu.py) held to the dense
restatements and to each other.

* poisson_ref.greedy_sparse == greedy and conflict_pairs == the upper triangle of conflicts on 3 000 uniform points at two radii, the
  lattice at the float above 0.0625, a cloud with NaN and inf coordinates, and 300 copies of one point.
* scale_ref.in_point_envelope is never wrong and tight enough, on point_neighbors_ref.scale_cloud() with r2 = float32(0.1)^2 at the
  scales 2^k, k in KS: no query it puts inside has restatement lists that differ from the image of scale 1; every query is inside at
  -31, -20, 30 and 62; at -70 fewer than 1 % of the queries are covariant and the lists hold subnormal d2; at -80 every count is 4 096.
* The Poisson restatement on 4 097 uniform points, min_dist2 = 0.002, seed 1: the flags of scale 1 at 2^k for k in (-62, -40, 40, 62, 64),
  other flags at -70 (min_dist2 is one subnormal ulp), every finite point kept at -75 (min_dist2 is 0)."""
import numpy as np
import pytest

import point_neighbors_ref as nref
import poisson_ref as pref
import scale_ref as sref

F32 = np.float32
KS = (-80, -70, -45, -31, -20, 0, 30, 62, 64)
R2 = float(F32(0.1) * F32(0.1))
FLT_MIN = np.finfo(F32).tiny


def scaled_r2(r2, k):
    with np.errstate(all="ignore"):
        return F32(np.ldexp(F32(r2), 2 * int(k)))


# ---- the sparse Poisson forms ----
def _bad_cloud(n=1500, seed=5):
    """test_poisson_gpu._bad_cloud: a tenth of the points with a NaN or an inf coordinate"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)).astype(F32)
    idx = rng.choice(n, n // 10, replace=False)
    p[idx, rng.integers(0, 3, len(idx))] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], F32), len(idx))
    p[idx[:5]] = np.nan
    return p


def _sparse_equals_dense(p, m, seed=0, priority=None):
    d2 = pref.d2_matrix(p)
    c = pref.conflicts(p, m, d2)
    i, j = np.nonzero(np.triu(c, 1))
    pairs = pref.conflict_pairs(p, m)
    assert pairs.dtype == np.int64 and np.array_equal(pairs, np.stack([i, j], 1)), (len(pairs), len(i))
    assert np.array_equal(pref.greedy_sparse(p, m, seed, priority), pref.greedy(p, m, seed, priority, d2))
    return len(pairs)


def test_sparse_forms_equal_the_dense_forms():
    p = np.random.default_rng(31).random((3000, 3)).astype(F32)
    few, many = _sparse_equals_dense(p, 0.0005, seed=2), _sparse_equals_dense(p, 0.01, seed=(1 << 63) + 5)
    assert 0 < few < many and many > 3000
    _sparse_equals_dense(p, 0.01, priority=np.random.default_rng(1).integers(0, 4, 3000).astype(np.uint32))
    lat = pref.lattice_case()
    assert _sparse_equals_dense(lat, F32(0.0625)) == 0
    assert _sparse_equals_dense(lat, np.nextafter(F32(0.0625), F32(1)), seed=3) == 3 * 7 * 64
    bad = _bad_cloud()
    for m in (0.002, 0.02):
        assert _sparse_equals_dense(bad, m, seed=3) > 0
    for none in (0.0, -1.0, np.nan):
        assert len(pref.conflict_pairs(bad, none)) == 0 and np.array_equal(pref.greedy_sparse(bad, none), pref.finite(bad))
    one = np.tile(np.asarray([[0.25, -3.0, 7.5]], F32), (300, 1))
    assert _sparse_equals_dense(one, 1.0, seed=1) == 300 * 299 // 2
    assert pref.greedy_sparse(one, 1.0, priority=np.full(300, 9, np.uint32)).nonzero()[0].tolist() == [0]


# ---- the neighbours' envelope ----
@pytest.fixture(scope="module")
def cloud():
    data, pts = nref.scale_cloud()
    assert (pts[0::8] == data[0::16]).all() and len(pts[0::8]) == 256
    full = {}
    for k in KS:
        off, rec, cnt = nref.neighbors(sref.scaled_points(pts, k), sref.scaled_points(data, k), max_dist2=scaled_r2(R2, k))
        full[k] = (off, rec, cnt)
    return data, pts, sref.point_measures(pts, data), full


def test_point_measures(cloud):
    data, pts, (min_dx, max_d2, fin), _ = cloud
    assert fin.all() and min_dx.shape == max_d2.shape == (len(pts),)
    ex = nref.exact_d2(pts[:64], data)
    assert np.array_equal(max_d2[:64], ex.max(1))
    dx = np.abs(pts[:64, None, :].astype(np.float64) - data[None].astype(np.float64))
    assert np.array_equal(min_dx[:64], np.where(dx > 0, dx, np.inf).min(axis=(1, 2))) and (min_dx > 0).all()
    bad = pts[:4].copy()
    bad[1, 2], bad[2, 0] = np.nan, np.inf
    m = sref.point_measures(bad, np.concatenate([data[:100], np.full((1, 3), np.nan, F32)]))
    assert m[2].tolist() == [True, False, False, True] and np.isfinite(m[1]).all()
    assert sref.in_point_envelope(m, R2, 0).tolist() == [True, False, False, True]
    assert not sref.in_point_envelope(m, np.asarray([np.inf, R2, R2, 0.0]), 0).any(), "a bound that is +inf or 0 is outside"
    empty = sref.point_measures(pts[:3], np.zeros((0, 3), F32))
    assert np.isposinf(empty[0]).all() and (empty[1] == 0).all()


def test_envelope_is_never_wrong_and_tight_enough(cloud):
    data, pts, measures, full = cloud
    n = len(pts)
    base = full[0]
    cov = {}
    for k in KS:
        inside = sref.in_point_envelope(measures, R2, k)
        cov[k] = sref.covariant_point_neighbors(base[:2], full[k][:2], k)
        print(f"k = {k}: {int(inside.sum())} of {n} inside, {int(cov[k].sum())} covariant")
        assert cov[k][inside].all(), (k, "a query inside the envelope has lists that are not the image of scale 1")
        if k in (-31, -20, 30, 62):
            assert inside.all(), (k, int(inside.sum()))
        if k in (-80, -70):
            assert not inside.any(), k
    assert cov[0].all() and cov[-45].all()
    rec70 = full[-70][1]["dist2"]
    assert cov[-70].sum() < n // 100 and ((rec70 > 0) & (rec70 < FLT_MIN)).sum() > 1000, "subnormal d2 in the lists at 2^-70"
    assert scaled_r2(R2, -80) == 0 and (full[-80][2] == len(data)).all(), "r2 and every d2 underflow to 0 at 2^-80"
    rec = full[-80][1][: len(data)]
    assert np.array_equal(rec["index"], np.arange(len(data))) and (rec["dist2"] == 0).all(), "ordered by index"
    inside64 = sref.in_point_envelope(measures, R2, 64)
    assert 0 < inside64.sum() < n, "at 2^64 the far pairs' d2 overflows for most queries, not for all"


# ---- Poisson ----
def test_poisson_flags_across_scale():
    p = np.random.default_rng(1).random((4097, 3)).astype(F32)
    p[7, 1], p[4000, 0] = np.nan, np.inf
    m = F32(0.002)
    d2 = pref.d2_matrix(p)
    want = pref.greedy(p, m, seed=1, d2=d2)
    assert 2000 < want.sum() < 3000
    for k in (-62, -40, 40, 62, 64):
        mk = scaled_r2(m, k)
        assert np.isfinite(mk) and mk > 0 and (mk >= FLT_MIN) == (k != -62), "at 2^-62 min_dist2 is subnormal, its leading bits kept"
        assert np.array_equal(pref.greedy(sref.scaled_points(p, k), mk, seed=1), want), k
    m70 = scaled_r2(m, -70)
    assert m70 == np.nextafter(F32(0), F32(1)), "one subnormal ulp"
    at70 = pref.greedy(sref.scaled_points(p, -70), m70, seed=1)
    assert not np.array_equal(at70, want) and at70.sum() > want.sum()
    assert scaled_r2(m, -75) == 0
    assert np.array_equal(pref.greedy(sref.scaled_points(p, -75), scaled_r2(m, -75), seed=1), pref.finite(p))

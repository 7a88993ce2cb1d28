"""No GPU: the neighbour and the winding-number queries across scale (include/cgrt.h "Neighbour queries" and "Winding numbers", DESIGN.md
5.26 and 5.25).  The CPU restatements the GPU tests hold the device to (neighbors_ref.neighbors, winding_ref.walk on the library's own
tree, read from host-only scenes) are swept over scene and queries multiplied by 2^k.

* Neighbours (cube, blob, dragon 5 k; 515 closest_ref.mixed_queries; k in test_point_scale_cpu.KS; the radius (0.05 extents)^2 * 2^2k
  where that is finite and non-zero, and +inf).  Wherever scale_ref.in_envelope says yes the full list at 2^k is the exact power-of-two
  image of the list at 1 (scale_ref.covariant_neighbors: the same count, the same prim_id order, dist2 * 2^2k), for every query, nothing
  left out; the envelope is non-vacuous at INSIDE_KS as in test_point_scale_cpu.py.  The two edges are asserted to be reached: at 2^62
  records with dist2 = +inf under the infinite radius (they tie on the key and are ordered by prim_id), at 2^-70 denormal dist2.
* Winding numbers (cube, blob, dodge, dragon 5 k; scale_ref.sign_queries(257) plus closest_ref.far_queries(129) -- 65 and 33 on dodge,
  whose walks cost ten times the others'; beta = 2 and +inf; k in WINDING_KS).  Wherever scale_ref.in_winding_envelope says yes -- and
  the BVH builder's record order is that of scale 1, asserted at MUST_BE_INSIDE -- the cluster tree is the power-of-two image
  (scale_ref.covariant_winding_tree), the three counters of the float32 walk over the inside points are those at scale 1, w has the bits
  it has at scale 1 (the winding number is scale-free: unchanged, not scaled), the float64 walk agrees with itself at scale 1 within 1e-12
  (float64 sums of a few thousand terms) and max |walk32 - walk64| stays under test_winding_gpu.py's soundness cap 1e-3.  The predicate
  must say yes for every point at k = -20, 20, 30, 33 on all four scenes and at -31 on cube, blob and dragon (INSIDE_LOW is what the GPU
  module imports).  The far family is dipole-only at beta = 2: no triangle is evaluated for it and its w is non-zero.
Each test prints its per-k table (DESIGN.md 5.25 and 5.26 carry a copy)."""
import numpy as np
import pytest

import closest_ref as cr
import neighbors_ref as nr
import scale_ref as sr
import winding_ref as wr
from test_point_scale_cpu import FAR, INSIDE_KS, KS, N, SEED

INF = float("inf")
RADIUS = 0.05  # of the extent
WINDING_KS = (-70, -42, -40, -31, -20, 0, 20, 30, 33, 40, 42, 62)
WINDING_SCENES = ("cube", "blob", "dodge", "dragon")
MUST_BE_INSIDE = (-20, 20, 30, 33)  # every point of every scene
INSIDE_LOW = {"cube": -31, "blob": -31, "dragon": -31, "dodge": -20}  # the lowest k of WINDING_KS at which every point is inside
NSIGN, NFAR = {"dodge": 65}, {"dodge": 33}
SOUND = 1e-3  # test_winding_gpu.py: the float32 restatement itself is sound on points off the surface
F64_NOISE = 1e-12


def _scene(pkg, scene_data, name):
    return pkg.scenes.make_dragon(5000) if name == "dragon" else scene_data(name)


# ---- neighbours ----
@pytest.mark.parametrize("name", ("cube", "blob", "dragon"))
def test_neighbour_lists_are_covariant_inside_the_envelope(pkg, scene_data, name):
    sd = _scene(pkg, scene_data, name)
    q = cr.mixed_queries(sd, N, SEED)
    fin = np.isfinite(q).all(axis=1)
    near = fin & (np.arange(N) % 5 != FAR)
    assert fin.sum() == N - 2
    r2 = np.float32(np.float32(RADIUS * nr.extent(sd)) ** 2)
    d0 = {}
    base = {"radius": nr.neighbors(sd, q, None, r2, dist2=d0), "inf": nr.neighbors(sd, q, None, INF, dist2=d0)}
    assert (np.diff(base["inf"][0])[fin] == sd.ntris).all() and not np.diff(base["inf"][0])[~fin].any()
    print(f"\n{name} ({sd.ntris} triangles, {int(fin.sum())} finite queries); shares in % of the finite queries; records of finite queries")
    print("    k  in-env  covariant: radius  +inf   largest count: radius  +inf   +inf dist2  denormal dist2")
    for k in KS:
        sk, qk = sr.scaled(sd, k), sr.scaled_points(q, k)
        env = sr.in_envelope(sk, qk)
        assert not env[~fin].any(), "non-finite points are outside"
        with np.errstate(all="ignore"):
            rk = np.float32(np.ldexp(r2, 2 * k))
        dk = {}
        row = {}
        for what, bound in (("radius", rk), ("inf", np.float32(INF))):
            if not (np.isfinite(bound) and bound > 0) and what == "radius":
                row[what] = None
                continue
            full = nr.neighbors(sk, qk, None, bound, dist2=dk)
            cov = sr.covariant_neighbors(base[what], full, k)
            bad = np.flatnonzero(env & ~cov)
            assert len(bad) == 0, (name, k, what, "not covariant inside the envelope", len(bad), int(bad[0]))
            assert not np.diff(full[0])[~fin].any(), "a non-finite point has no neighbours"
            assert not np.isnan(full[1]["dist2"]).any(), "a NaN never qualifies"
            row[what] = (cov, full)
        cov_i, full_i = row["inf"]
        d2 = full_i[1]["dist2"]
        n_inf, n_den = int(np.isposinf(d2).sum()), int(((d2 > 0) & (d2 < sr.FLT_MIN)).sum())
        pct = lambda m: 100.0 * (m & fin).sum() / fin.sum()  # noqa: E731
        rad = row["radius"]
        print(f"  {k:3d}  {pct(env):6.1f}  " + (f"{pct(rad[0]):17.1f}" if rad else f"{'--':>17}") + f"  {pct(cov_i):5.1f}  "
              + (f"{int(np.diff(rad[1][0]).max()):21d}" if rad else f"{'--':>21}") + f"  {int(np.diff(full_i[0]).max()):5d}  {n_inf:10d}  {n_den:14d}")
        if k in INSIDE_KS:
            must = near if k == 30 else fin
            assert env[must].all(), (name, k, "queries outside the envelope", int((must & ~env).sum()))
            assert rad is not None
        if k == 62:
            assert n_inf > 0, "the sweep reaches +inf dist2 that qualifies under the infinite radius"
            off, rec = full_i
            for i in np.flatnonzero(fin)[:64]:
                mine = rec[off[i] : off[i + 1]]
                tied = mine["prim_id"][np.isposinf(mine["dist2"])]
                assert (np.diff(tied.astype(np.int64)) > 0).all(), "records that tie at +inf are ordered by prim_id"
        if k == -70:
            assert n_den > 0, "the sweep reaches denormal dist2"


# ---- winding numbers ----
def _tree(pkg, sd):
    sc = pkg.Scene(sd, device=-1)  # host-only
    try:
        tree = sc.debug_winding_tree()
    finally:
        sc.close()
    return tree, wr.records(sd, tree)


def winding_points(sd, name):
    """(points, first index of the far family)."""
    ns, nf = NSIGN.get(name, 257), NFAR.get(name, 129)
    return np.ascontiguousarray(np.concatenate([sr.sign_queries(sd, ns, 11), cr.far_queries(sd, nf, 15)]), np.float32), ns


@pytest.mark.parametrize("name", WINDING_SCENES)
def test_winding_walk_is_scale_free_inside_the_envelope(pkg, scene_data, name):
    sd = _scene(pkg, scene_data, name)
    q, nsign = winding_points(sd, name)
    n = len(q)
    assert np.isfinite(q).all()
    far = np.arange(n) >= nsign
    tree0, recs0 = _tree(pkg, sd)
    base = {}
    for beta in (2.0, INF):
        w32, work = wr.walk(tree0, recs0, q, beta, np.float32)
        w64, work64 = wr.walk(tree0, recs0, q, beta, np.float64)
        assert work == work64
        base[beta] = (w32, w64, work)
    # the far family is dipole-only at beta = 2
    fw, fwork = wr.walk(tree0, recs0, q[far], 2.0, np.float32)
    print(f"\n{name} ({len(recs0)} triangles, {nsign} sign and {n - nsign} far points); far family at beta 2: counters {fwork}")
    assert fwork[2] == 0 and fwork[0] == fwork[1] > 0 and (fw != 0).all() and np.isfinite(fw).all(), (name, fwork)
    print("    k  in-env %  order  tree  bit-covariant % (beta 2, inf)  max |w32 - w64| (beta 2)  NaN (beta 2)")
    lowest = None
    for k in WINDING_KS:
        sk, qk = sr.scaled(sd, k), sr.scaled_points(q, k)
        tree, recs = _tree(pkg, sk)
        order = np.array_equal(tree0["record_prims"], tree["record_prims"])
        pred = sr.in_winding_envelope(sk, qk)
        env = pred & order  # (the record order is the BVH builder's: where it differs from scale 1 the scale is outside)
        tree_cov = sr.covariant_winding_tree(tree0, tree, k)
        if k in MUST_BE_INSIDE or k == 0 or k == INSIDE_LOW[name]:
            assert order, (name, k, "the record order differs from scale 1")
            assert pred.all(), (name, k, "points outside the envelope", int((~pred).sum()))
        if pred.all() and order and lowest is None:
            lowest = k
        shares = []
        for beta in (2.0, INF):
            w0_32, w0_64, work0 = base[beta]
            if beta == 2.0 or env.any():
                w32, work = wr.walk(tree, recs, qk, beta, np.float32)
                same = sr._bits_eq(w32, w0_32)
                shares.append(f"{100.0 * same.mean():5.1f}")
            else:
                shares.append("   --")
            if beta == 2.0:
                w64, _ = wr.walk(tree, recs, qk, beta, np.float64)
                with np.errstate(all="ignore"):
                    err = np.abs(w32.astype(np.float64) - w64)
                worst, nans = (float(np.nanmax(err)) if np.isfinite(err).any() else float("nan")), int(np.isnan(w32).sum())
            if not env.any():
                continue
            assert tree_cov, (name, k, "the cluster tree is not the power-of-two image")
            bad = np.flatnonzero(env & ~same)
            assert len(bad) == 0, (name, k, beta, "w is not the float of scale 1 inside the envelope", len(bad), int(bad[0]))
            if env.all():
                assert work == work0, (name, k, beta, "counters", work, work0)
            else:  # the counters are sums: over the inside points only
                sub = wr.walk(tree, recs, qk[env], beta, np.float32)[1]
                assert sub == wr.walk(tree0, recs0, q[env], beta, np.float32)[1], (name, k, beta, "counters of the inside points")
            if beta != 2.0:
                w64, _ = wr.walk(tree, recs, qk, beta, np.float64)
            assert np.abs(w64[env] - w0_64[env]).max() <= F64_NOISE, (name, k, beta, "float64 walk", float(np.abs(w64[env] - w0_64[env]).max()))
            sound = float(np.abs(w32[env].astype(np.float64) - w64[env]).max())
            assert sound <= SOUND, (name, k, beta, "max |walk32 - walk64| inside the envelope", sound)
        print(f"  {k:3d}  {100.0 * env.mean():8.1f}  {int(order):5d}  {int(tree_cov):4d}  {shares[0]:>16} {shares[1]}  {worst:24.2e}  {nans:12d}")
    assert lowest == INSIDE_LOW[name], (name, "the lowest k at which every point is inside", lowest)

"""No GPU: the point queries across scale (closest points, crossings, signed distance; include/cgrt.h "Envelope" paragraphs, DESIGN.md 5.20,
5.21, 5.24).  The CPU restatements the GPU tests hold the device to (closest_ref.brute, crossings_ref.reference, sdf_ref.reference) are
swept over scene and queries multiplied by 2^k, k in KS.

* Covariance.  Wherever scale_ref.in_envelope says yes the result at 2^k is the exact power-of-two image of the result at 1 (scale_ref's
  predicates), for every query, nothing left out.  The envelope is not vacuous: at k = -20, 0, 20 every finite query and every finite ray
  of the three scenes is inside; at k = 30 every query of the four near families is (the far family, 100 extents away, is not: there E *
  M = 2^67 and va, vb, vc overflow -- those queries still come out covariant because a vertex region decides them, which the envelope does
  not promise; likewise every finite ray of the six families whose origins lie in the grown box, the camera standing 4.3 extents from
  the cube).  On dodge, whose sliver triangles ((2 * area)^2 = 2^-68) put its lower edge at 2^-11, the restatement is asserted NOT to be
  covariant at 2^-20 and to be at 2^-10.  Each test prints its table: per k the share inside the envelope, the share covariant per
  entry, the largest ratio of the two float64 quantities to K, the share of misses and of non-finite dist2 (DESIGN.md 5.20 and 5.24
  carry a copy).
* Float64 truth.  At every k, for every query inside the envelope, test_closest_cpu's two quantities stay within K * 2^-24 * scale * 2^k
  (K imported from there, scale = max(1, |p|inf, the scene's largest |coordinate|) at k = 0).  The float64 distances are computed once at
  k = 0 and multiplied by 2^k: float64 neither overflows nor underflows anywhere in |k| <= 62, so that is what closest_ref.dist64 of the
  scaled scene returns.
* The lemma at the edges: lb2 <= dist2 in float32, no slack, a NaN never greater, on the cube and the blob at 2^-70, 2^-31, 2^33, 2^62 --
  denormals, NaN and +inf included (asserted to be there at -70 and 62).
* Sign against geometry: on the closed meshes (cube, dragon) `inside` equals |float64 winding number| > 0.5 and |sdf| the float64 distance
  for every point farther than 1e-4 extents from the surface.  blob, monkey and dodge are NOT closed: their SDF tests pin the definition,
  not geometry."""
import numpy as np
import pytest

import closest_ref as cr
import crossings_ref as xr
import scale_ref as sr
import sdf_ref
from test_closest_cpu import K

KS = (-70, -40, -31, -20, 0, 20, 30, 33, 40, 62)
INSIDE_KS = (-20, 0, 20, 30)  # must lie in the envelope (at 30: the near families)
N = 515
SEED = 11
SCENES = ("cube", "blob", "dragon")
FAR = 4  # closest_ref.mixed_queries: query i belongs to family i % 5, the far family is the last
CAMERA = 0  # crossings_ref.mixed_rays: ray i belongs to family i % 7, the camera's rays are the first

_cache = {}


def _scene(pkg, scene_data, name):
    return pkg.scenes.make_dragon(5000) if name == "dragon" else scene_data(name)


def _base(pkg, orc, scene_data, name):
    """The scene, its queries and rays and the three restatements' results at k = 0, once."""
    if name not in _cache:
        sd = _scene(pkg, scene_data, name)
        q = cr.mixed_queries(sd, N, SEED)
        rays = xr.mixed_rays(pkg, orc, sd, N, SEED)
        _cache[name] = dict(sd=sd, q=q, rays=rays, closest=cr.brute(sd, q), crossings=xr.reference(orc, sd, rays),
                            sdf=sdf_ref.reference(orc, sd, q, pkg.INSIDE_DIRECTIONS), D=cr.dist64(sd, q))
    return _cache[name]


@pytest.mark.parametrize("name", SCENES)
def test_restatements_are_covariant_and_true_inside_the_envelope(pkg, orc, scene_data, name):
    b = _base(pkg, orc, scene_data, name)
    sd, q, rays, D = b["sd"], b["q"], b["rays"], b["D"]
    fin, rfin = np.isfinite(q).all(axis=1), np.isfinite(rays[:, 0:3]).all(axis=1)
    near = fin & (np.arange(N) % 5 != FAR)
    near_rays = rfin & (np.arange(N) % 7 != CAMERA)
    assert fin.sum() == N - 2 and rfin.sum() == N - 1
    D64 = D.min(axis=1)
    scale = np.maximum(1.0, np.maximum(np.abs(q.astype(np.float64)).max(axis=1), cr.scene_scale(sd)))
    print(f"\n{name} ({sd.ntris} triangles, {int(fin.sum())} finite queries, {int(rfin.sum())} finite rays, K = {K:.2f}); shares in %")
    print("    k  in-env  covariant: closest crossings sdf   ratio/K: distance triangle   misses  non-finite dist2")
    for k in KS:
        sk, qk, rk = sr.scaled(sd, k), sr.scaled_points(q, k), sr.scaled_rays(rays, k)
        env, renv = sr.in_envelope(sk, qk), sr.in_envelope(sk, rk[:, 0:3])
        assert not env[~fin].any() and not renv[~rfin].any(), "non-finite points are outside"
        got = cr.brute(sk, qk)
        cov_c = sr.covariant_closest(b["closest"], got, k)
        cov_x = sr.covariant_crossings(b["crossings"], xr.reference(orc, sk, rk), k)
        cov_s = sr.covariant_sdf(b["sdf"], sdf_ref.reference(orc, sk, qk, pkg.INSIDE_DIRECTIONS), k)
        # the two float64 quantities of test_closest_cpu, in units of 2^-24 * scale * 2^k
        unit = np.ldexp(2.0 ** -24 * scale, k)
        hit = fin & (got["prim_id"] != cr.NO_PRIM)
        with np.errstate(all="ignore"):
            r1 = np.abs(np.sqrt(got["dist2"].astype(np.float64)) - np.ldexp(D64, k)) / unit
            r2 = (np.ldexp(D[np.arange(N), np.where(hit, got["prim_id"], 0)], k) - np.ldexp(D64, k)) / unit
        r1, r2 = np.where(hit, r1, np.inf), np.where(hit, r2, np.inf)  # (a miss of an unbounded query is infinitely far off)
        pct = lambda m, of: 100.0 * m.sum() / of.sum()  # noqa: E731
        print(f"  {k:3d}  {pct(env, fin):6.1f}  {pct(cov_c & fin, fin):18.1f} {pct(cov_x & rfin, rfin):9.1f} {pct(cov_s & fin, fin):5.1f}"
              f"  {np.nanmax(r1[fin]) / K:17.3g} {np.nanmax(r2[fin]) / K:8.3g}  {pct(fin & ~hit, fin):7.1f}  {pct(hit & ~np.isfinite(got['dist2']), fin):7.1f}")
        for what, cov, inside in (("closest", cov_c, env), ("crossings", cov_x, renv), ("sdf", cov_s, env)):
            bad = np.flatnonzero(inside & ~cov)
            assert len(bad) == 0, (name, k, what, "not covariant inside the envelope", len(bad), int(bad[0]))
        assert hit[env].all(), (name, k, "an unbounded query inside the envelope finds a triangle")
        if env.any():
            assert r1[env].max() <= K, (name, k, "distance", float(r1[env].max()), int(np.flatnonzero(env)[r1[env].argmax()]))
            assert r2[env].max() <= K, (name, k, "returned triangle", float(r2[env].max()), int(np.flatnonzero(env)[r2[env].argmax()]))
        if k in INSIDE_KS:
            must = near if k == 30 else fin
            assert env[must].all(), (name, k, "queries outside the envelope", int((must & ~env).sum()))
            rmust = near_rays if k == 30 else rfin
            assert renv[rmust].all(), (name, k, "rays outside the envelope", int((rmust & ~renv).sum()))


def test_dodge_leaves_the_envelope_at_its_slivers(pkg, scene_data):
    """dodge's smallest non-zero |ab x ac|^2 is 2^-68: at 2^-20 it is subnormal, in_envelope says no for every query, and closest_ref.brute
    is indeed not covariant there; at 2^-10 every finite query is inside and covariant."""
    sd = scene_data("dodge")
    q = cr.mixed_queries(sd, 257, SEED)
    fin = np.isfinite(q).all(axis=1)
    r0 = cr.brute(sd, q)
    assert 2.0 ** -70 < sr._triangle_measures(sd)[1] < 2.0 ** -66
    for k, inside in ((-20, False), (-10, True)):
        sk, qk = sr.scaled(sd, k), sr.scaled_points(q, k)
        env = sr.in_envelope(sk, qk)
        cov = sr.covariant_closest(r0, cr.brute(sk, qk), k)
        print(f"dodge, 2^{k}: {int(env.sum())} of {int(fin.sum())} finite queries inside the envelope, {int((fin & ~cov).sum())} not covariant")
        if inside:
            assert env[fin].all() and cov[fin].all(), k
        else:
            assert not env.any() and (fin & ~cov).any(), (k, "the envelope's lower edge excludes something real")


@pytest.mark.parametrize("k", (-70, -31, 33, 62))
@pytest.mark.parametrize("name", ("cube", "blob"))
def test_box_lower_bound_never_exceeds_dist2_at_the_edges(pkg, orc, scene_data, name, k):
    """test_closest_cpu.test_box_lower_bound_never_exceeds_dist2 on the scaled scene: the tree search is exact only if the lemma holds
    among denormals, NaN and inf too."""
    b = _base(pkg, orc, scene_data, name)
    sd, q = sr.scaled(b["sd"], k), sr.scaled_points(b["q"], k)  # (with the NaN and the inf point)
    a, bb, c = cr.tri_verts(sd)
    assert np.isfinite(a).all() and np.isfinite(bb).all() and np.isfinite(c).all()
    lo, hi = np.minimum(np.minimum(a, bb), c), np.maximum(np.maximum(a, bb), c)
    rng = np.random.default_rng(17)
    ext = (hi - lo).max()
    step = max(1, (1 << 18) // len(a))
    tiny, nonfinite = 0, 0
    for s in range(0, len(q), step):
        p = q[s : s + step, None, :]
        _, d2, _, _, _ = cr.closest_tri32(p, a, bb, c)
        assert not (cr.box_lb2(lo, hi, p) > d2).any(), (name, k, "own box")
        for _ in range(3):
            g = rng.random((2,) + lo.shape).astype(np.float32) * np.float32(ext) * (rng.random((2,) + lo.shape) < 0.67)
            glo, ghi = (lo - g[0]).astype(np.float32), (hi + g[1]).astype(np.float32)
            assert (glo <= lo).all() and (ghi >= hi).all()
            assert not (cr.box_lb2(glo, ghi, p) > d2).any(), (name, k, "grown box")
        tiny += int(((d2 > 0) & (d2 < sr.FLT_MIN)).sum())
        nonfinite += int((~np.isfinite(d2[np.isfinite(p).all(axis=-1)[:, 0]])).sum())
    if k == -70:
        assert tiny > 0, "the sweep reaches denormal dist2"
    if k == 62:
        assert nonfinite > 0, "the sweep reaches inf / NaN dist2 of finite queries"


@pytest.mark.parametrize("name", ("cube", "dragon"))
def test_sign_against_the_winding_number_on_closed_meshes(pkg, orc, scene_data, name):
    sd = _scene(pkg, scene_data, name)
    assert sr.is_closed(sd)
    pts = sr.sign_queries(sd, 1025, 61)
    assert len(pts) == 1025
    ext = sr.extent(sd)
    D64 = cr.dist64(sd, pts).min(axis=1)
    w = sr.winding64(sd, pts)
    sdf, inside = sdf_ref.reference(orc, sd, pts, pkg.INSIDE_DIRECTIONS)
    keep = D64 > 1e-4 * ext
    scale = np.maximum(1.0, np.maximum(np.abs(pts.astype(np.float64)).max(axis=1), cr.scene_scale(sd)))
    ratio = np.abs(np.abs(sdf.astype(np.float64)) - D64) / (2.0 ** -24 * scale)
    truth = np.abs(w) > 0.5
    print(f"{name}: {100.0 * (~keep).mean():.2f} % left out, {100.0 * truth[keep].mean():.1f} % inside, winding numbers within "
          f"{np.abs(np.abs(w[keep]) - truth[keep]).max():.1e} of 0 / 1, largest ||sdf| - D64| {ratio[keep].max():.3f} units (K = {K:.2f})")
    assert (~keep).sum() <= 0.02 * len(pts)
    assert (np.abs(np.abs(w[keep]) - truth[keep]) <= 1e-6).all(), "a closed mesh: the winding number is 0 or +-1 off the surface"
    assert truth[keep].any() and (~truth[keep]).any()
    bad = np.flatnonzero(keep & (inside != truth))
    assert len(bad) == 0, (name, len(bad), int(bad[0]), pts[bad[0]], float(w[bad[0]]))
    assert (np.signbit(sdf) == inside).all()
    assert ratio[keep].max() <= K, (name, float(ratio[keep].max()), int(np.flatnonzero(keep)[ratio[keep].argmax()]))


def test_which_fixtures_are_closed(pkg, scene_data):
    """`inside` has a geometric meaning on closed meshes only.  Whoever swaps a fixture learns here which tests carry it."""
    assert sr.is_closed(scene_data("cube"))
    for n in (5000, 20_000):
        assert sr.is_closed(pkg.scenes.make_dragon(n)), n
    for name in ("blob", "monkey", "dodge"):
        assert not sr.is_closed(scene_data(name)), name

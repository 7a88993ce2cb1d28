"""No GPU: the surface family across scale -- the barycentric weights (include/cgrt.h cgrt_hit_barycentrics*, "Envelope")
and the host sampling table (include/cgrt.h "Surface sampling").  Scene, ray origins and t are multiplied by 2^k, k in KS.
The items are scale_ref.surface_items: hits made without a tracer (the weights never walk the tree, so the tracer's limits do not apply),
one in eight on an edge, one in sixteen on a vertex.

* The predicate is sound: every item scale_ref.in_surface_envelope puts inside at k has surface_ref.weights at 2^k bit-equal to the
  weights at 1 (scale_ref.covariant_weights), on all five scenes at every k.
* The predicate is not vacuous: at k in ALL_INSIDE every item of every scene is inside, at 2^-40 at least 90 %, at 2^-75 none, at 2^64
  none of the cube's.  These are conditions on the inputs, not tolerances.
* The edges are reached by the restatement: NaN weights (cube, 2^64), weights that differ from scale 1 for more than half of the items
  (monkey, 2^-62), at least 100 items with a weight that is exactly 0 (cube, dodge).
* The host sampling table at every k: Scene(device=-1).triangle_areas() and debug_sample_table() equal sampling_ref.table of the scaled
  scene -- areas by bits, the total by bytes, thresholds and last exactly -- and the cases of TABLE_EDGES are reached: scenes that become
  empty for sampling, areas that overflow and are counted as 0 while `last` stays, thousands of subnormal areas, a `last` that moves.
Each test prints its per-k table (include/cgrt.h's example range and DESIGN.md 5.19 carry a copy).  Building the host-only scenes at
every k here is also what keeps the GPU module from meeting a builder problem first."""
import numpy as np
import pytest

import sampling_ref as sref
import scale_ref as sr
import surface_ref

SCENES = ("cube", "cornell", "monkey", "blob", "dodge")
TABLE_SCENES = ("cube", "cornell", "monkey", "dodge")
N, SEED = 4097, 5
KS = (-75, -70, -56, -40, -31, -20, 0, 30, 33, 62, 63, 64, 66)
ALL_INSIDE = (-31, -20, 30, 33, 62, 63)  # every item of every scene
MOSTLY_INSIDE, SHARE = -40, 0.90
ZERO_WEIGHTS = {"cube": 100, "dodge": 100}  # at least this many items with a weight that is exactly 0


def items(sd):
    """(rays, prim, hit flags, the measures of scale_ref.surface_measures) of the module's items on sd."""
    rays, prim = sr.surface_items(sd, N, SEED)
    return rays, prim, np.ones(len(prim), np.uint32), sr.surface_measures(sd, rays, prim)


def weights_at(sd, rays, prim, hit, k):
    sk, rk = sr.scaled(sd, k), sr.scaled_rays(rays, k)
    return surface_ref.weights(sk, rk, rk[:, 6], prim, hit)


# ---- 1. the predicate: sound, not vacuous, and the edges reached ----
@pytest.mark.parametrize("name", SCENES)
def test_weights_have_the_bits_of_scale_one_inside_the_envelope(scene_data, name):
    sd = scene_data(name)
    rays, prim, hit, measures = items(sd)
    edge, vertex = np.arange(N) % 8 == 1, np.arange(N) % 16 == 2
    w0 = surface_ref.weights(sd, rays, rays[:, 6], prim, hit)
    assert np.isfinite(w0).all()
    zeros = int((w0 == 0).any(axis=1).sum())
    print(f"\n{name} ({sd.ntris} triangles, {N} items, {int(edge.sum())} on an edge, {int(vertex.sum())} on a vertex); {zeros} items with a weight of exactly 0")
    print("    k  in-env %  bit-covariant %  NaN items")
    if name in ZERO_WEIGHTS:
        assert zeros >= ZERO_WEIGHTS[name], (name, zeros)
    for k in KS + ((-62,) if name == "monkey" else ()):
        wk = weights_at(sd, rays, prim, hit, k)
        env, cov = sr.in_surface_envelope(measures, k), sr.covariant_weights(w0, wk)
        nans = int(np.isnan(wk).any(axis=1).sum())
        print(f"  {k:3d}  {100.0 * env.mean():8.2f}  {100.0 * cov.mean():15.2f}  {nans:9d}")
        bad = np.flatnonzero(env & ~cov)
        assert len(bad) == 0, (name, k, "not the bits of scale 1 inside the envelope", len(bad), int(bad[0]))
        if k in ALL_INSIDE or k == 0:
            assert env.all(), (name, k, "items outside the envelope", int((~env).sum()))
            assert env[edge].all() and env[vertex].all()
        if k == MOSTLY_INSIDE:
            assert env.mean() >= SHARE, (name, k, float(env.mean()))
        if k == -75 or (k == 64 and name == "cube"):
            assert not env.any(), (name, k, int(env.sum()))
        if k == 64 and name == "cube":
            assert nans > 0, "the sweep reaches NaN weights"
        if k == -62 and name == "monkey":
            assert cov.mean() < 0.5, "the sweep reaches weights that differ from scale 1 for more than half of the items"


# ---- 2. the host sampling table at every k ----
def library_table(pkg, sd):
    sc = pkg.Scene(sd, device=-1)
    try:
        areas, total = sc.triangle_areas()
        tab = sc.debug_sample_table()
    finally:
        sc.close()
    return areas, total, tab["thresholds"], tab["last"]


def assert_same_table(lib, ref, what):
    assert np.array_equal(lib[0].view(np.uint32), ref[0].view(np.uint32)), (what, "areas")
    assert np.float64(lib[1]).tobytes() == np.float64(ref[1]).tobytes(), (what, "total")
    assert lib[2].dtype == np.uint32 and np.array_equal(lib[2], ref[2]), (what, "thresholds")
    assert lib[3] == ref[3], (what, "last")


def table_is_that_of_scale_one(tab, tab0):
    return bool(np.array_equal(tab[2], tab0[2]) and tab[3] == tab0[3])


def _subnormal(a):
    return int(((a > 0) & (a < sr.FLT_MIN)).sum())


# (scene, k) -> what the restatement's table must show there
TABLE_EDGES = {
    ("cube", 64): lambda a, T, last, same: last == sref.NO_PRIM,
    ("cube", 66): lambda a, T, last, same: last == sref.NO_PRIM,
    ("cornell", 64): lambda a, T, last, same: int((a == 0).sum()) == 10 and last == 31,
    ("cube", 63): lambda a, T, last, same: same,
    ("cornell", 63): lambda a, T, last, same: same,
    ("monkey", 63): lambda a, T, last, same: same,
    ("dodge", 63): lambda a, T, last, same: same,
    ("cube", -56): lambda a, T, last, same: same,
    ("cornell", -56): lambda a, T, last, same: same,
    ("monkey", -56): lambda a, T, last, same: same,
    ("dodge", -56): lambda a, T, last, same: _subnormal(a) > 16000 and not same,
    ("monkey", -70): lambda a, T, last, same: last == 967 and int((a == 0).sum()) == 328,
}
TABLE_EDGES.update({(name, -75): (lambda a, T, last, same: last == sref.NO_PRIM) for name in TABLE_SCENES})
SAME_TABLE = {63: TABLE_SCENES, -56: ("cube", "cornell", "monkey")}  # where the table is that of scale 1 (the GPU module imports this)
assert all(TABLE_EDGES[(name, k)](None, None, None, True) for k, names in SAME_TABLE.items() for name in names)


@pytest.mark.parametrize("name", TABLE_SCENES)
def test_host_sampling_table_equals_the_restatement_at_every_k(pkg, scene_data, name):
    sd = scene_data(name)
    ref0 = sref.table(sd)
    assert ref0[3] == sd.ntris - 1
    print(f"\n{name} ({sd.ntris} triangles)")
    print("    k  zero areas  subnormal areas        last  longest run of one threshold  table of scale 1")
    for k in KS:
        sk = sr.scaled(sd, k)
        ref = sref.table(sk)
        assert_same_table(library_table(pkg, sk), ref, (name, k))
        a, _, T, last = ref
        same = table_is_that_of_scale_one(ref, ref0)
        edges = np.flatnonzero(np.diff(T.astype(np.int64)) != 0)
        run = int(np.diff(np.concatenate([[-1], edges, [len(T) - 1]])).max())
        print(f"  {k:3d}  {int((a == 0).sum()):10d}  {_subnormal(a):15d}  {last:10d}  {run:28d}  {int(same):16d}")
        if (name, k) in TABLE_EDGES:
            assert TABLE_EDGES[(name, k)](a, T, last, same), (name, k, "the edge case is not reached")
        if last == sref.NO_PRIM:
            assert not T.any() and ref[1] == 0.0
            rec, _ = sref.sample(sk, 5, tab=ref)
            assert (rec["prim_id"] == sref.NO_PRIM).all()


# ---- 3. the host-only scenes the GPU module needs build at every k ----
def unit_square(pkg):
    """The unit square as two right triangles (test_surface_grad_gpu.py's)."""
    pn = np.zeros((4, 6), np.float32)
    pn[:, 5] = 1
    pn[:, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    return pkg.scenes.SceneData(pos_nrm=pn, tri=np.asarray([[0, 1, 2], [1, 3, 2]], np.uint32), tri_mesh=np.zeros(2, np.uint32),
                                materials=np.asarray([[0.5, 0.5, 0.5, 0, 0, 0, 1, 1]], np.float32), name="square")


FRAME_KS = (-70, -31, 30, 62, 64)
EXTRA_KS = {"dodge": (-66,)}


@pytest.mark.parametrize("name", ("blob", "dodge", "square"))
def test_host_only_scenes_build_at_every_k(pkg, scene_data, name):
    sd = unit_square(pkg) if name == "square" else scene_data(name)
    for k in (FRAME_KS if name == "square" else KS + EXTRA_KS.get(name, ())):
        sk = sr.scaled(sd, k)
        sc = pkg.Scene(sk, device=-1)
        try:
            areas, total = sc.triangle_areas()
        finally:
            sc.close()
        assert np.array_equal(areas.view(np.uint32), sref.areas(sk).view(np.uint32)), (name, k)

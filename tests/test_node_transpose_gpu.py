"""GPU tests of the TRANSPOSED 4-wide nodes (cgrt_layout.h SubNode): a ray picks the near and the far planes of a
node's four children by ADDRESS -- quarter 2a + s_a and 2a + 1 - s_a, s_a the sign of the clamped direction component -- where the
step used to select them from {lower, upper} pairs.  The arithmetic is the same fma on the same operands, so

  * every walker (certified, exact, brute force) still answers like the oracle, bit for bit, for rays of EVERY sign octant inside one
    wave, axis-parallel and face-diagonal directions (zero components: the clamped sign; outside RayFast::fd), -0.0 and denormal
    components, in each kernel shape a ray list can take (QUAD4, LANE16, LANE64 by its length);
  * a frame visits exactly the nodes, triangles and certificate boxes it visited before the change: the counters of
    cgrt_count_primary equal the figures the parent commit produced on the GPU (tests/golden/node_transpose_counts.json);
  * closest-point queries (closest_kernels.hip reads the same nodes) and a depth-2 shaded frame (compact primary kernel, shadow and
    mirror lists) still match their CPU references.
"""
import json
import os

import numpy as np
import pytest

import closest_ref as cr
from conftest import GOLDEN, same_bits
from test_parity_gpu import _assert_hits_equal, _rays

pytestmark = pytest.mark.gpu

NDIR = 4096
LENGTHS = (64, 4096, 9_000, 140_000)  # QUAD4; the base list; LANE16; LANE64 (trace_kernels.hip quad_shape_for: 8192 and 131072 part them)
COUNTERS = ("sub_visits", "tri_tests", "cert_boxes", "tree_rays", "fallback_rays")


def _directions():
    """NDIR unit-ish directions: a Fibonacci sphere permuted so that every 64 consecutive ones (a wave) hold all eight octants, with
    the 6 axis-parallel and 12 face-diagonal directions and components that are -0.0 or denormal written over the first slots."""
    i = np.arange(NDIR, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / NDIR
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)
    d = d[np.random.RandomState(17).permutation(NDIR)]
    special = []
    for a in range(3):
        for s in (1.0, -1.0):
            v = np.zeros(3, np.float32)
            v[a] = s
            special.append(v)
    for a in range(3):
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                v = np.zeros(3, np.float32)
                v[(a + 1) % 3], v[(a + 2) % 3] = s0, s1
                special.append(v / np.float32(np.sqrt(2.0)))
    den = np.float32(1e-41)  # a denormal
    for a in range(3):
        for tiny in (np.float32(-0.0), den, -den):
            v = np.array([0.6, -0.64, 0.48], np.float32)
            v[a] = tiny
            special.append(v)
            special.append(-v)  # (-(-0.0) = +0.0, the other clamped sign)
    special = np.asarray(special, np.float32)
    # spread over the list, one every 61 slots: they share waves with ordinary rays of all octants
    d[(np.arange(len(special)) * 61) % NDIR] = special
    octant = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
    for w in range(0, NDIR, 64):
        assert len(np.unique(octant[w : w + 64])) == 8, "every octant inside every wave"
    return d


def _origins(sd, orc, n):
    """n points strictly inside the root box: its centre first, the others spread over the middle half."""
    _, boxes = orc.OracleScene(sd).nodes()
    lo, hi = boxes[0, :3].astype(np.float64), boxes[0, 3:].astype(np.float64)
    u = np.random.RandomState(3).uniform(0.25, 0.75, size=(n, 3))
    u[0] = 0.5
    return (lo + u * (hi - lo)).astype(np.float32)


def _ray_list(sd, orc, n):
    d = _directions()
    o = _origins(sd, orc, (n + NDIR - 1) // NDIR)
    r7 = np.empty((len(o) * NDIR, 7), np.float32)
    r7[:, 0:3] = np.repeat(o, NDIR, axis=0)
    r7[:, 3:6] = np.tile(d, (len(o), 1))
    r7[:, 6] = np.float32(np.inf)
    return r7[:n]


_cache = {}


def _scene(pkg, orc, scene_data, name):
    """(SceneData, Scene, the longest ray list, the oracle's answer for it, the oracle's brute-force answer for the base list), made once per scene."""
    if name not in _cache:
        sd = pkg.scenes.make_dragon(5000) if name == "dragon5000" else scene_data(name)
        r7 = _ray_list(sd, orc, max(LENGTHS))
        o = orc.OracleScene(sd)
        ref = o.intersect(r7)
        # the reference's loop over every triangle (ray_tracing.cpp:202-213) is an answer of its own: it finds hits the reference's
        # tree misses and meets the triangles of a tie in load order -- the device's brute force is held to the oracle's
        ref_brute = o.intersect(r7[:NDIR], brute_force=True)
        ref.setflags(write=False)
        ref_brute.setflags(write=False)
        _cache[name] = (sd, pkg.Scene(sd), r7, ref, ref_brute)
    return _cache[name]


@pytest.fixture()
def forced_fast_tree(pkg):
    pkg.set_fast_tree(1)  # the thin-leaf scene is below the size at which a fast tree is built by default
    yield
    pkg.set_fast_tree(-1)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["dragon5000", "cornell"])
def test_all_sign_octants_every_walker(pkg, orc, scene_data, forced_fast_tree, name, n):
    sd, sc, r7, ref, ref_brute = _scene(pkg, orc, scene_data, name)
    assert sc.num_subnodes() > 0 and sc.walk() == 1
    rays = _rays(pkg, r7[:n])
    want = ref[:n]
    assert 0.05 < (want["hit"] == 1).mean(), "the rays start inside the model's box and most directions meet it"
    hits, normals = sc.intersect(rays)
    _assert_hits_equal(hits, normals, want, f"{name} n={n} certified walk")
    sc.set_walk(False)
    try:
        hits, normals = sc.intersect(rays)
    finally:
        sc.set_walk(True)
    _assert_hits_equal(hits, normals, want, f"{name} n={n} exact walk")
    if n <= NDIR:  # (the brute force tests every triangle per ray: the base list covers every direction)
        hits, normals = sc.intersect_brute(rays)
        _assert_hits_equal(hits, normals, ref_brute[:n], f"{name} n={n} brute force")


def _count_scene(pkg, name):
    kind, ntris = name.split("_")
    return (pkg.scenes.make_dragon if kind == "dragon" else pkg.scenes.make_dragon_irregular)(int(ntris))


@pytest.mark.parametrize("name", ["dragon_5000", "dragon_87000", "irregular_20000"])
def test_same_visits_as_the_parent(pkg, name):
    """Equality is exact: the step's arithmetic did not change, so no ray enters another child, in another order."""
    with open(os.path.join(GOLDEN, "node_transpose_counts.json")) as f:
        want = json.load(f)["counts"][name]
    sc = pkg.Scene(_count_scene(pkg, name))
    W = H = 256
    got = sc.count_primary(pkg.scenes.default_camera(W, H), W, H)
    print(name, {k: got[k] for k in COUNTERS})
    assert got["rays"] == W * H and got["sub_visits"] > 0
    assert {k: int(got[k]) for k in COUNTERS} == {k: int(want[k]) for k in COUNTERS}


def test_closest_points_and_a_shaded_frame(pkg, orc):
    sd = pkg.scenes.make_dragon(5000)
    sc = pkg.Scene(sd)
    assert sc.num_subnodes() > 0
    q = cr.mixed_queries(sd, 1025, 11)
    tree, ref = sc.closest_points(q), cr.brute(sd, q)
    assert (tree["prim_id"] == ref["prim_id"]).all()
    for f in ("point", "dist2", "bary"):
        assert same_bits(tree[f], ref[f]).all(), f
    W = H = 128
    cam = pkg.scenes.default_camera(W, H)
    rgb, st = sc.render(cam, W, H, max_level=2)
    refrgb, nrays = orc.OracleScene(sd).render(cam, W, H, sd.point_lights, max_level=2)
    err = np.abs(rgb.astype(np.float64) - refrgb).max()
    assert err <= 1e-5, f"max abs RGB error {err}"  # BASELINE.json north_star: final pixel RGB within 1e-5 abs
    assert st["primary_rays"] + st["shadow_rays"] + st["reflection_rays"] == nrays and st["primary_rays"] == W * H
    assert (refrgb.sum(1) > 0).mean() > 0.02

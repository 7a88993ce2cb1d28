"""What tools/fuzz_queries.py rests on, checked without a device: its generators are deterministic and make what they claim (ties,
duplicates, every scene kind and triangle count), the shared soup still makes the parity fuzz's scenes, and the references of its
reference legs stay inside their own bounds on its own scenes -- so that on the device a violation points at the kernel."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import closest_ref as cr  # noqa: E402
import point_neighbors_ref as pnr  # noqa: E402
import scale_ref  # noqa: E402
from test_fuzz_queries_gpu import ITERATIONS, WINDING_F32_ERR, WINDING_F32_ERR_OFF_SURFACE, seeds  # noqa: E402


@pytest.fixture(scope="module")
def fq(pkg):
    import fuzz_queries

    return fuzz_queries


def _scene_bytes(sd):
    return b"".join(np.ascontiguousarray(getattr(sd, f)).tobytes() for f in ("pos_nrm", "tri", "tri_mesh", "materials"))


def test_generators_are_deterministic(fq):
    for seed in seeds():
        for it in range(ITERATIONS):
            a, b = fq.make_scene(seed, it), fq.make_scene(seed, it)
            assert (a.kind, a.tris, a.k) == (b.kind, b.tris, b.k) and _scene_bytes(a.sd) == _scene_bytes(b.sd), (seed, it)
            assert fq.make_points(a, seed, it).tobytes() == fq.make_points(b, seed, it).tobytes(), (seed, it)
            assert fq.make_rays(a, seed, it).tobytes() == fq.make_rays(b, seed, it).tobytes(), (seed, it)
            c, d = fq.make_cloud(seed, it), fq.make_cloud(seed, it)
            for f in ("data", "points", "radius2"):
                assert getattr(c, f).tobytes() == getattr(d, f).tobytes(), (seed, it, f)
            assert (c.kind, c.m, c.n, c.k, c.step, c.r2, c.cell, c.skip, c.frame_k) == (d.kind, d.m, d.n, d.k, d.step, d.r2, d.cell, d.skip, d.frame_k)
    assert _scene_bytes(fq.make_scene(seeds()[0], 0).sd) != _scene_bytes(fq.make_scene(seeds()[0], 1).sd)


def test_the_shared_soup_makes_the_parity_fuzz_scenes(pkg):
    """tools/fuzz_scenes.soup(rng) against the loop fuzz_parity had, restated: the committed parity seeds keep their scenes (the first
    scenes of seeds 101 and 202 among them)."""
    import fuzz_scenes

    def old_soup(rng):
        nmesh = rng.randint(1, 30)
        rows, tris, tm = [], [], []
        for m in range(nmesh):
            nt = int(rng.choice([1, 2, 5, 30, 200, 1500, 6000]))
            c = rng.uniform(-0.8, 0.8, 3)
            sz = rng.uniform(0.02, 0.5)
            for _ in range(nt):
                p0 = c + rng.uniform(-sz, sz, 3)
                tri = np.stack([p0, p0 + rng.uniform(-0.1, 0.1, 3), p0 + rng.uniform(-0.1, 0.1, 3)])
                kind = rng.randint(0, 40)
                if kind == 0:
                    tri[2] = tri[1]
                elif kind == 1 and tris:
                    tri = np.asarray(rows[-3:])[:, 0:3]
                elif kind == 2:
                    tri[:, rng.randint(0, 3)] = tri[0, 0]
                base = len(rows)
                nrm = rng.normal(size=(3, 3))
                for k in range(3):
                    rows.append(np.concatenate([tri[k], nrm[k] / np.linalg.norm(nrm[k])]))
                tris.append((base, base + 1, base + 2))
                tm.append(m)
        return pkg.scenes.SceneData(pos_nrm=np.asarray(rows, np.float32), tri=np.asarray(tris, np.uint32), tri_mesh=np.asarray(tm, np.uint32),
                                    materials=rng.uniform(0, 1, (nmesh, 8)).astype(np.float32))

    for s in (101 * 100003, 202 * 100003, 12):  # (fuzz_parity seeds iteration `it` of seed s with s * 100003 + it)
        rng = np.random.RandomState(s)
        rng.randint(0, 5)  # the scene kind is drawn first
        want = old_soup(rng)
        rng = np.random.RandomState(s)
        rng.randint(0, 5)
        got = fuzz_scenes.soup(rng)
        assert _scene_bytes(got) == _scene_bytes(want) and got.ntris == want.ntris > 0
    capped = fuzz_scenes.soup(np.random.RandomState(3), max_tris=513, sizes=(1, 2, 5))
    assert capped.ntris == 513 and capped.nmesh > 100 and int(capped.tri_mesh.max()) == capped.nmesh - 1


def test_lattice_scenes_and_clouds_hold_ties(fq):
    """A 65-triangle lattice scene: duplicates are present, and at least 5 % of the fuzz's own queries have two triangles at a
    bit-equal dist2 -- also at the smallest one, where the tie rule decides the closest record.  Lattice clouds alike."""
    import fuzz_scenes

    base = fuzz_scenes.lattice(np.random.default_rng(65), 65)
    fs = fq.FuzzScene("lattice", "lattice", 65, 0, base)
    a, b, c = cr.tri_verts(fs.sd)
    tri = np.concatenate([a, b, c], axis=1)
    dup = len(tri) - len(np.unique(tri, axis=0))
    assert 1 <= dup <= 0.12 * len(tri), dup
    P = np.concatenate([fq.make_points(fs, 65, it) for it in range(8)])
    P = P[np.isfinite(P).all(axis=1)]
    with np.errstate(all="ignore"):
        _, d2, _, _, _ = cr.closest_tri32(P[:, None, :], a, b, c)
    s = np.sort(np.where(np.isnan(d2), np.inf, d2), axis=1)
    any_tie = (np.isfinite(s[:, 1:]) & (s[:, 1:] == s[:, :-1])).any(axis=1).mean()
    best_tie = (np.isfinite(s[:, 0]) & (s[:, 0] == s[:, 1])).mean()
    print(f"{len(P)} queries, {dup} duplicated triangles: {any_tie:.3f} with two triangles at one dist2, {best_tie:.3f} at the smallest")
    assert any_tie >= 0.05 and best_tie >= 0.05
    cloud = next(c for c in (fq.make_cloud(seeds()[0], it) for it in range(64)) if c.kind == "lattice" and c.m >= 300 and c.n >= 63)
    assert len(cloud.data) - len(np.unique(cloud.data, axis=0)) > 0
    with np.errstate(all="ignore"):
        s = np.sort(pnr.d2_matrix(cloud.points[np.isfinite(cloud.points).all(axis=1)], cloud.data), axis=1)
    assert (np.isfinite(s[:, 1:]) & (s[:, 1:] == s[:, :-1])).any(axis=1).mean() >= 0.05


def test_every_kind_and_count_occurs_in_the_committed_seeds(fq):
    kinds, counts, ckinds, sizes, steps = set(), set(), set(), set(), set()
    for seed in seeds():
        for it in range(ITERATIONS):
            fs = fq.make_scene(seed, it)
            kinds.add(fs.kind)
            counts.add(fs.tris)
            assert fs.tris == 0 or fs.sd.ntris == fs.tris, (seed, it, fs.describe())
            c = fq.make_cloud(seed, it)
            ckinds.add(c.kind), sizes.add(c.m), steps.add(c.step)
    assert kinds == set(fq.KINDS) and counts >= set(fq.TRI_COUNTS), (kinds, counts)
    assert ckinds == set(fq.CLOUD_KINDS) and sizes == set(fq.CLOUD_SIZES) and {-4, 4} <= steps, (ckinds, sizes, steps)


def test_reference_bounds_hold_on_the_cpu(fq):
    """The reference legs on the CPU, with the restatements in the device's place, over the reference subsamples of the committed seeds.
    Measured and printed: how far closest_ref.brute is from the float64 distance inside the envelope, in units of the header's 5.66
    bound (tools/fuzz_queries.py CLOSEST_F32_RATIO is held to it: slivers exceed the header's figure, which the header now says), and
    how far the float32 winding number is from float64, over all queries inside its envelope and over those off the surface (the
    constants of the GPU test are held to both).  Asserted: at scales 2^0, 2^-8 and 2^7 the envelopes leave at least half of a
    subsample's queries, so that the bounded comparisons cannot pass by emptiness -- on scenes without holes (a non-finite vertex
    leaves a scene of one or two triangles nothing to measure, and every float64 winding number a NaN) and lists of 8 queries or more."""
    worst_ratio, worst_w, worst_off, subsamples, filtered = 0.0, 0.0, 0.0, 0, 0
    for seed in seeds():
        for it in range(ITERATIONS):
            fs = fq.make_scene(seed, it)
            if fs.sd.ntris > fq.REF_TRIS:
                continue
            subsamples += 1
            P = fq.make_points(fs, seed, it)[: fq.REF_QUERIES]
            with np.errstate(all="ignore"):
                rec = cr.brute(fs.sd, P)
            ratio, ok = fq.closest_error(fs.sd, P, rec)
            err, okw, off = fq.winding_error(fs.sd, P, fq.winding_restated(fs.sd, P))
            e_off = float(err[off].max(initial=0.0))
            print(f"seed {seed} iteration {it} {fs.describe()}: {len(P)} queries, {int(ok.sum())} in the closest envelope, worst "
                  f"{ratio.max():.3f} of the bound; {int(okw.sum())} in the winding envelope, worst error {err.max():.3g}, "
                  f"{int(off.sum())} of them off the surface, worst error {e_off:.3g}")
            worst_ratio, worst_w, worst_off = max(worst_ratio, float(ratio.max())), max(worst_w, float(err.max())), max(worst_off, e_off)
            if fs.k in (0, -8, 7) and fs.kind != "holes" and len(P) >= 8:
                assert 2 * int(ok.sum()) >= len(P) and 2 * int(okw.sum()) >= len(P), (seed, it, int(ok.sum()), int(okw.sum()), len(P))
                filtered += 1
    print(f"{subsamples} subsamples: closest worst {worst_ratio:.3f} of the bound; float32 winding number worst error {worst_w!r}, off the surface {worst_off!r}")
    assert subsamples >= 6 and filtered >= 2
    assert worst_ratio <= fq.CLOSEST_F32_RATIO <= 2.0 * worst_ratio, (worst_ratio, fq.CLOSEST_F32_RATIO)
    assert np.isfinite(worst_w) and worst_w <= WINDING_F32_ERR <= 2.0 * worst_w, (worst_w, WINDING_F32_ERR)
    assert 0 < worst_off <= WINDING_F32_ERR_OFF_SURFACE <= 2.0 * worst_off, (worst_off, WINDING_F32_ERR_OFF_SURFACE)

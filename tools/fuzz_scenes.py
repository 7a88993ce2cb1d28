"""Random scenes the fuzz tools share (tools/fuzz_parity.py, tools/fuzz_queries.py).  numpy only: nothing here touches a device.
`soup` is fuzz_parity's multi-mesh soup, moved here unchanged: called as soup(rng) it makes the draws it always made, so the committed
parity seeds (tests/fuzz_seeds.txt) keep their scenes (tests/test_fuzz_queries_cpu.py holds that against a restatement of the old
loop).  fuzz_queries asks for an exact triangle count and for soups of many tiny meshes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as e  # noqa: E402

pkg = e.load_package()
SOUP_SIZES = (1, 2, 5, 30, 200, 1500, 6000)


def soup(rng, max_tris=None, sizes=SOUP_SIZES):
    """Meshes of random size at random places: one triangle in 40 has zero area, one repeats the triangle before it, one is
    axis-aligned.  rng: a np.random.RandomState.  max_tris=None: 1 .. 29 meshes, as drawn.  With max_tris the soup has exactly that
    many triangles: the last mesh is cut short, and further meshes are drawn while the soup is still smaller."""
    nmesh = rng.randint(1, 30)
    rows, tris, tm = [], [], []
    m = 0
    while m < nmesh or (max_tris is not None and len(tris) < max_tris):
        if max_tris is not None and len(tris) >= max_tris:
            break
        nt = int(rng.choice(list(sizes)))
        c = rng.uniform(-0.8, 0.8, 3); sz = rng.uniform(0.02, 0.5)
        for _ in range(nt):
            if max_tris is not None and len(tris) >= max_tris:
                break
            p0 = c + rng.uniform(-sz, sz, 3)
            tri = np.stack([p0, p0 + rng.uniform(-0.1, 0.1, 3), p0 + rng.uniform(-0.1, 0.1, 3)])
            kind = rng.randint(0, 40)
            if kind == 0: tri[2] = tri[1]
            elif kind == 1 and tris: tri = np.asarray(rows[-3:])[:, 0:3]
            elif kind == 2: tri[:, rng.randint(0, 3)] = tri[0, 0]  # axis-aligned
            base = len(rows); nrm = rng.normal(size=(3, 3))
            for k in range(3): rows.append(np.concatenate([tri[k], nrm[k] / np.linalg.norm(nrm[k])]))
            tris.append((base, base + 1, base + 2)); tm.append(m)
        m += 1
    return pkg.scenes.SceneData(pos_nrm=np.asarray(rows, np.float32), tri=np.asarray(tris, np.uint32), tri_mesh=np.asarray(tm, np.uint32),
                                materials=rng.uniform(0, 1, (m, 8)).astype(np.float32))


def lattice(g, ntris):
    """ntris triangles whose vertex coordinates are all multiples of 1/4 in [-1, 1]: every dist2 and every t of a lattice query is exact,
    so they tie across many triangles.  Seven in ten are small (edges of one lattice step).  5-10 % of the triangles (at least one
    from two triangles on) are exact copies of an earlier one under another prim_id, at most 64 copies of any one; 2 % are given zero
    area on top of those the draw makes.  g: a np.random.Generator.  One mesh, three vertices of its own per triangle."""
    T = int(ntris)
    v0 = g.integers(-4, 5, (T, 3))
    small = g.random(T) < 0.7
    e1 = np.where(small[:, None], g.integers(-1, 2, (T, 3)), g.integers(-8, 9, (T, 3)))
    e2 = np.where(small[:, None], g.integers(-1, 2, (T, 3)), g.integers(-8, 9, (T, 3)))
    e1[(e1 == 0).all(1)] = (1, 0, 0)
    e2[(e2 == 0).all(1)] = (0, 1, 0)
    v = np.stack([v0, np.clip(v0 + e1, -4, 4), np.clip(v0 + e2, -4, 4)], axis=1)  # (T, 3, 3) integers
    flat = g.random(T) < 0.02
    v[flat, 2] = v[flat, 1]
    nd = int(round(T * g.uniform(0.05, 0.10)))
    if T >= 2:
        nd = max(nd, 1)
    root, copies = np.arange(T), np.ones(T, np.int64)
    for i in np.sort(g.choice(np.arange(1, T), nd, replace=False)) if nd else ():
        for _ in range(8):
            j = int(root[g.integers(0, i)])
            if copies[j] < 64:
                v[i], root[i] = v[j], j
                copies[j] += 1
                break
    nrm = g.normal(size=(3 * T, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pn = np.concatenate([v.reshape(-1, 3) * 0.25, nrm], axis=1).astype(np.float32)
    return pkg.scenes.SceneData(pos_nrm=pn, tri=np.arange(3 * T, dtype=np.uint32).reshape(T, 3), tri_mesh=np.zeros(T, np.uint32),
                                materials=g.uniform(0, 1, (1, 8)).astype(np.float32))


def punched(sd, g):
    """The scene with one NaN and one infinite vertex coordinate, in two different vertices that triangles use."""
    pn = np.asarray(sd.pos_nrm, np.float32).copy()
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    a = int(tri[g.integers(0, len(tri)), 0])
    cand = tri.reshape(-1)[tri.reshape(-1) != a]
    b = int(cand[g.integers(0, len(cand))])
    pn[a, g.integers(0, 3)] = np.nan
    pn[b, g.integers(0, 3)] = np.inf if g.integers(0, 2) else -np.inf
    return pkg.scenes.SceneData(pos_nrm=pn, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials)

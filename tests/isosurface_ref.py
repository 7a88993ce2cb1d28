"""A numpy restatement of include/cgrt.h "Iso-surfaces" (marching tetrahedra on a scalar grid), vectorised over the grid, with the mesh
checks the tests share: directed edges, Euler characteristic, signed volume.  float32 throughout, one rounding per operation.
`carrying_edges` is the vertex order on its own; `compose_slabs` builds the mesh of a grid too large to restate whole from z-slabs of it.

The triangle table is DERIVED here by rule and never typed in:
  * one or three inside corners: one triangle on the three edges at the odd corner, the edges in ascending order;
  * two inside corners a < b with outside corners c < d: the quad (ac, ad, bd, bc), split along ac-bd into (ac, ad, bd) and (ac, bd, bc);
  * a triangle whose normal does not point from the inside corners' mean to the outside corners' mean has its last two vertices swapped.
"""
from __future__ import annotations

import re

import numpy as np

F32 = np.float32
TETS = ((0, 1, 3, 7), (0, 5, 1, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 6, 4, 7))
CORNERS = np.asarray([(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)], np.int64)  # corner c = x + 2 y + 4 z -> (dx, dy, dz)


def _edge(a: int, b: int):
    return (min(a, b), max(a, b))


def derive_table() -> dict:
    """{mask: [triangle, ...]}, a triangle three tetrahedron edges (pa, pb), pa < pb corner positions, in the order they are written."""
    P = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float64)  # a positively oriented tetrahedron
    assert np.linalg.det(P[1:] - P[0]) > 0
    table = {}
    for m in range(16):
        ins = [k for k in range(4) if (m >> k) & 1]
        out = [k for k in range(4) if not (m >> k) & 1]
        if len(ins) in (0, 4):
            table[m] = []
            continue
        if len(ins) == 2:
            (a, b), (c, d) = ins, out
            tris = [(_edge(a, c), _edge(a, d), _edge(b, d)), (_edge(a, c), _edge(b, d), _edge(b, c))]
        else:
            odd = ins[0] if len(ins) == 1 else out[0]
            tris = [tuple(sorted(_edge(odd, k) for k in range(4) if k != odd))]
        want = P[out].mean(0) - P[ins].mean(0)
        fixed = []
        for t in tris:
            q = [(P[e[0]] + P[e[1]]) * 0.5 for e in t]
            if np.dot(np.cross(q[1] - q[0], q[2] - q[0]), want) < 0:
                t = (t[0], t[2], t[1])
            fixed.append(t)
        table[m] = fixed
    return table


def parse_header_table(text: str) -> dict:
    """The table as include/cgrt.h prints it ("  m: (01,02,03) ..."), in derive_table's form."""
    table = {0: [], 15: []}
    for m, body in re.findall(r"(?<![\d,(])(\d{1,2}): ((?:\(\d\d,\d\d,\d\d\) ?)+)", text):
        tris = [tuple((int(e[0]), int(e[1])) for e in t.split(",")) for t in re.findall(r"\((\d\d,\d\d,\d\d)\)", body)]
        assert int(m) not in table, f"row {m} printed twice"
        table[int(m)] = tris
    return table


def _table_arrays():
    tab = derive_table()
    n = np.zeros(16, np.int64)
    e = np.zeros((16, 2, 3, 2), np.int64)
    for m, tris in tab.items():
        n[m] = len(tris)
        for k, t in enumerate(tris):
            e[m, k] = t
    return n, e


def carrying_edges(values, iso=0.0, inside_above=False):
    """(owner, etype): the vertex-carrying edges of values ((nz, ny, nx) float32, every dim >= 2) in the vertex order -- by the owner's
    point index, then by edge type."""
    v = np.ascontiguousarray(np.asarray(values, F32))
    nz, ny, nx = v.shape
    iso = F32(iso)
    fin = np.isfinite(v)
    ins = fin & ((v > iso) if inside_above else (v < iso))
    carries = np.zeros((nz, ny, nx, 7), bool)
    for e in range(7):
        dx, dy, dz = CORNERS[e + 1]
        A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        carries[A + (e,)] = fin[A] & fin[B] & (ins[A] != ins[B])
    return np.nonzero(carries.reshape(-1, 7))  # row-major: by owner, then by edge type


def isosurface(values, origin, spacing, iso=0.0, inside_above=False, want_work=False):
    """(verts (nv, 3) float32, tris (nt, 3) uint32) of values ((nz, ny, nx) float32); want_work: also the four counters
    (cells that emit, tetrahedra that emit, vertices, triangles)."""
    v = np.ascontiguousarray(np.asarray(values, F32))
    nz, ny, nx = v.shape
    o, sp = np.asarray(origin, F32).reshape(3), np.asarray(spacing, F32).reshape(3)
    iso = F32(iso)
    empty = (np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32))
    if min(nx, ny, nz) < 2:
        return empty + ((0, 0, 0, 0),) if want_work else empty
    N = nx * ny * nz
    fin = np.isfinite(v)
    ins = fin & ((v > iso) if inside_above else (v < iso))
    owner, etype = carrying_edges(v, iso, inside_above)
    nv = len(owner)
    vid = np.full((N, 7), -1, np.int64)
    vid[owner, etype] = np.arange(nv)
    d = CORNERS[etype + 1]
    idx = [owner % nx, (owner // nx) % ny, owner // (nx * ny)]
    flat = v.reshape(-1)
    vA, vB = flat[owner], flat[owner + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny]
    with np.errstate(all="ignore"):
        t = (iso - vA) / (vB - vA)
        t = np.where(t >= F32(0), t, F32(0)).astype(F32)
        t = np.where(t > F32(1), F32(1), t).astype(F32)
        verts = np.empty((nv, 3), F32)
        for c in range(3):
            pA = o[c] + idx[c].astype(F32) * sp[c]
            pB = o[c] + (idx[c] + d[:, c]).astype(F32) * sp[c]
            verts[:, c] = pA + t * (pB - pA)
    assert verts.dtype == F32 and t.dtype == F32

    # cells, in the order of their corner 0's point index
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cell = ((cz * ny + cy) * nx + cx).reshape(-1)
    off = CORNERS[:, 0] + CORNERS[:, 1] * nx + CORNERS[:, 2] * nx * ny
    finf, insf = fin.reshape(-1), ins.reshape(-1)
    tab_n, tab_e = _table_arrays()
    tets = np.asarray(TETS, np.int64)
    cfin = np.stack([finf[cell + off[c]] for c in range(8)], 1)  # (C, 8)
    cins = np.stack([insf[cell + off[c]] for c in range(8)], 1)
    mask = np.zeros((len(cell), 6), np.int64)
    ok = np.ones((len(cell), 6), bool)
    for ti in range(6):
        for k in range(4):
            mask[:, ti] |= cins[:, tets[ti, k]].astype(np.int64) << k
            ok[:, ti] &= cfin[:, tets[ti, k]]
    ntri = np.where(ok, tab_n[mask], 0)  # (C, 6)
    live = ntri.sum(1) > 0
    cell, mask, ntri = cell[live], mask[live], ntri[live]
    rows = tab_e[mask]  # (C', 6, 2, 3, 2): corner positions
    which = np.arange(6)[None, :, None, None]
    ca, cb = tets[which, rows[..., 0]], tets[which, rows[..., 1]]  # cell corners
    lo, hi = np.minimum(ca, cb), np.maximum(ca, cb)
    index = vid[cell[:, None, None, None] + off[lo], hi - lo - 1]  # (C', 6, 2, 3)
    exists = np.arange(2)[None, None, :] < ntri[:, :, None]  # (C', 6, 2)
    tris = index[exists]  # row-major: by cell, then tetrahedron, then table position
    assert (tris >= 0).all(), "a table vertex lies on an edge that carries no vertex"
    res = (verts, tris.astype(np.uint32).reshape(-1, 3))
    if want_work:
        res += ((int(live.sum()), int((ntri > 0).sum()), nv, len(tris)),)
    return res


def compose_slabs(values_slabs, z0s, origin, spacing, iso=0.0, inside_above=False):
    """(verts, tris) of a whole grid from z-slabs of it: slab s holds the layers [z0s[s], z0s[s] + len(values_slabs[s])) of the grid on
    (origin, spacing), the slabs ascend and do not overlap, and no edge outside the slabs carries a vertex: every layer between two
    slabs lies on the side of the level on which a slab's last layer and, unless it is layer 0, its first layer lie (that these outer
    layers are finite and of one side is asserted; the layers in between are the caller's).  Vertices are
    ordered by owner index and triangles by cell index, both z-major, so the whole grid's mesh is the slabs' vertices concatenated, then
    the slabs' triangles concatenated with every later slab's indices shifted by the vertices before it.
    Precondition, asserted: every coordinate origin.c + i * spacing.c involved is exact in float32, so that a slab's own origin
    origin.z + z0 * spacing.z and the positions built on it have the bits the whole grid gives them."""
    o, sp = np.asarray(origin, F32).reshape(3), np.asarray(spacing, F32).reshape(3)
    iso = F32(iso)
    verts, tris, base, last = [], [], 0, 0
    for val, z0 in zip(values_slabs, z0s):
        val = np.ascontiguousarray(np.asarray(val, F32))
        nz, ny, nx = val.shape
        z0 = int(z0)
        assert z0 >= last, "the slabs ascend and do not overlap"
        last = z0 + nz
        for c, n in ((0, nx), (1, ny), (2, z0 + nz)):
            i = np.arange(n)
            exact = float(o[c]) + i.astype(np.float64) * float(sp[c])
            assert n <= 1 << 24 and np.array_equal((o[c] + i.astype(F32) * sp[c]).astype(np.float64), exact), "a grid coordinate is not exact"
            assert np.array_equal((i.astype(F32) * sp[c]).astype(np.float64), i.astype(np.float64) * float(sp[c]))
        for layer in ([val[0]] if z0 > 0 else []) + [val[-1]]:
            side = (layer > iso) if inside_above else (layer < iso)
            assert np.isfinite(layer).all() and (side.all() or not side.any()), "a slab's outer layer is crossed"
        so = o.copy()
        so[2] = o[2] + F32(z0) * sp[2]
        v, t = isosurface(val, so, sp, iso=iso, inside_above=inside_above)
        verts.append(v)
        tris.append((t.astype(np.int64) + base).astype(np.uint32))
        base += len(v)
    return np.concatenate(verts), np.concatenate(tris)


# ---- mesh checks
def directed_edges(tris) -> np.ndarray:
    """every directed edge a -> b of the triangles as a * 2^32 + b"""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    return np.concatenate([(t[:, k] << 32) | t[:, (k + 1) % 3] for k in range(3)])


def is_closed(tris) -> bool:
    """every directed edge occurs exactly once, and its reverse exactly once"""
    e = directed_edges(tris)
    if len(e) == 0:
        return True
    u, n = np.unique(e, return_counts=True)
    rev = ((u & 0xFFFFFFFF) << 32) | (u >> 32)
    return bool((n == 1).all() and np.array_equal(np.sort(rev), u))


def euler_characteristic(nverts: int, tris) -> int:
    e = directed_edges(tris)
    a, b = e >> 32, e & 0xFFFFFFFF
    und = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b))
    return int(nverts) - len(und) + len(np.asarray(tris).reshape(-1, 3))


def unreferenced(nverts: int, tris) -> int:
    return int(nverts) - len(np.unique(np.asarray(tris).reshape(-1)))


def signed_volume(verts, tris) -> float:
    p = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0)


# ---- the fields of the tests
def grid_axes(origin, spacing, dims):
    o, sp = np.asarray(origin, F32), np.asarray(spacing, F32)
    return [o[c] + np.arange(int(dims[c]), dtype=F32) * sp[c] for c in range(3)]


def field(name: str, dims, box=1.2, seed=0):
    """(values (nz, ny, nx) float32, origin, spacing) of a named field on [-box, box]^3"""
    nx, ny, nz = (int(x) for x in dims)
    origin = np.full(3, -box, F32)
    spacing = np.asarray([2.0 * box / max(n - 1, 1) for n in (nx, ny, nz)], F32)
    ax = grid_axes(origin, spacing, dims)
    X, Y, Z = ax[0][None, None, :].astype(np.float64), ax[1][None, :, None].astype(np.float64), ax[2][:, None, None].astype(np.float64)
    if name == "sphere":
        val = np.sqrt(X * X + Y * Y + Z * Z) - 1.0
    elif name == "torus":
        val = np.sqrt((np.sqrt(X * X + Y * Y) - 1.0) ** 2 + Z * Z) - 0.4
    elif name == "gyroid":
        k = 2.5
        val = np.sin(k * X) * np.cos(k * Y) + np.sin(k * Y) * np.cos(k * Z) + np.sin(k * Z) * np.cos(k * X) + 0.0 * X
    elif name == "noise":
        val = np.random.default_rng(seed).uniform(-1.0, 1.0, (nz, ny, nx))
    elif name == "constant":
        val = np.full((nz, ny, nx), 0.25)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(np.broadcast_to(val, (nz, ny, nx)).astype(F32)), origin, spacing


def integer_field():
    """|x| + |y| + |z| - 2 on the 7^3 lattice -3..3: its zeros fall exactly on grid points"""
    a = np.arange(-3, 4, dtype=np.float64)
    val = np.abs(a)[None, None, :] + np.abs(a)[None, :, None] + np.abs(a)[:, None, None] - 2.0
    return val.astype(F32), np.full(3, -3.0, F32), np.ones(3, F32)

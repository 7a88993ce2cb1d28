"""The numpy restatement of include/cgrt.h "Grid fields, the adjoint of the sampler" (cgrt_sample_grid_grad*).  The cell
of a point is grid_field_ref.cell, the forward's own; the eight contributions are computed in float32 arrays, so every operation rounds
on its own, in the header's order.  Per element of the volume the module gives the float64 sum of the previous content and the float32
contributions (`exact`), their number m and S = |a| + sum |c| -- what the header's bound is stated in -- and a sequential float32 sum in
point order, corners in the order x + 2 y + 4 z (`sequential`: one of the orders the library may take, and the stand-alone checker's)."""
from __future__ import annotations

import numpy as np

import grid_field_ref as gref

F = np.float32
U = 2.0 ** -24
K = 10  # include/cgrt.h: |c - C| <= K u (|gv| W + sum_c |gg_c / spacing.c| W_c)


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def contributions(origin, spacing, dims, points, grad_value=None, grad_gradient=None, clamp=False):
    """-> (inside (n,) bool, index (n, 8) int64 into the flat values, c (n, 8) float32).  Column k = x + 2 y + 4 z.  Rows of outside
    points hold zeros (their grads are not read).  A contribution that is zero is not added by the library."""
    if grad_value is None and grad_gradient is None:
        raise ValueError("one of grad_value and grad_gradient must be given")
    nx, ny, nz = (int(x) for x in dims)
    sp = np.asarray(spacing, F).reshape(3)
    inside, i, f = gref.cell(origin, spacing, (nx, ny, nz), points, clamp)
    n = len(inside)
    base = (i[:, 2] * ny + i[:, 1]) * nx + i[:, 0]
    w = [np.stack([F(1) - f[:, c], f[:, c]], axis=1).astype(F) for c in range(3)]
    gv = None if grad_value is None else np.asarray(grad_value, F).reshape(n)
    index = np.zeros((n, 8), np.int64)
    out = np.zeros((n, 8), F)
    with np.errstate(all="ignore"):
        q = None if grad_gradient is None else (np.asarray(grad_gradient, F).reshape(n, 3) / sp[None, :]).astype(F)
        for k in range(8):
            x, y, z = k & 1, (k >> 1) & 1, k >> 2
            index[:, k] = base + x + y * nx + z * nx * ny
            wxy = w[0][:, x] * w[1][:, y]
            terms = []
            if gv is not None:
                terms.append(gv * (wxy * w[2][:, z]))
            if q is not None:
                terms.append((q[:, 0] if x else -q[:, 0]) * (w[1][:, y] * w[2][:, z]))
                terms.append((q[:, 1] if y else -q[:, 1]) * (w[0][:, x] * w[2][:, z]))
                terms.append((q[:, 2] if z else -q[:, 2]) * wxy)
            s = terms[0]
            for t in terms[1:]:
                s = s + t
            assert s.dtype == F
            out[:, k] = s
    out = np.where(inside[:, None], out, F(0)).astype(F)
    index = np.where(inside[:, None], index, 0)
    return inside, index, out


def adjoint(origin, spacing, dims, points, grad_value=None, grad_gradient=None, clamp=False, previous=None):
    """-> dict: 'exact' float64 (nz, ny, nx), the sum of `previous` (float32, default zeros) and the float32 contributions; 'm' int64, the
    contributions per element (zeros are not contributions); 'S' float64, |previous| + sum |c|; 'sequential' float32, previous with the
    contributions added one by one in point order; 'contributions' = contributions(...)."""
    nx, ny, nz = (int(x) for x in dims)
    inside, index, c = contributions(origin, spacing, dims, points, grad_value, grad_gradient, clamp)
    prev = np.zeros((nz, ny, nx), F) if previous is None else np.ascontiguousarray(previous, F).reshape(nz, ny, nx)
    added = inside[:, None] & (c != 0)  # a NaN is not equal to 0 and is added
    idx, val = index[added], c[added]  # point-major, corner-minor: the sequential order
    exact = prev.astype(np.float64).reshape(-1).copy()
    S = np.abs(prev.astype(np.float64)).reshape(-1).copy()
    m = np.zeros(nx * ny * nz, np.int64)
    seq = prev.reshape(-1).copy()
    with np.errstate(all="ignore"):
        np.add.at(exact, idx, val.astype(np.float64))
        np.add.at(S, idx, np.abs(val.astype(np.float64)))
        np.add.at(m, idx, 1)
        np.add.at(seq, idx, val)  # unbuffered: one float32 addition per entry, in order
    shape = (nz, ny, nx)
    return {"exact": exact.reshape(shape), "m": m.reshape(shape), "S": S.reshape(shape), "sequential": seq.reshape(shape),
            "contributions": (inside, index, c)}


def bound(res):
    """The header's bound per element: gamma(m + 1) S + (m + 1) 2^-126."""
    return gamma(res["m"] + 1) * res["S"] + (res["m"] + 1) * 2.0 ** -126


def check(got, res, previous=None, what=""):
    """got (nz, ny, nx) float32 against the header: elements with m = 0 keep their previous bits; the others lie within bound(res) of
    res['exact'], a NaN or infinite sum being met by the same.  Raises AssertionError with the worst element."""
    got = np.asarray(got, F).reshape(res["m"].shape)
    prev = np.zeros_like(got) if previous is None else np.asarray(previous, F).reshape(got.shape)
    untouched = res["m"] == 0
    assert np.array_equal(got.view(np.uint32)[untouched], prev.view(np.uint32)[untouched]), (what, "an element without contributions moved")
    ex, fin = res["exact"], np.isfinite(res["exact"])
    assert np.array_equal(np.isnan(got), np.isnan(ex)), (what, "NaN elements differ")
    inf = np.isinf(ex)
    assert np.array_equal(got[inf].astype(np.float64), ex[inf]), (what, "infinite elements differ")
    err = np.abs(got.astype(np.float64) - ex)[fin & ~untouched]
    lim = bound(res)[fin & ~untouched]
    if len(err):
        ratio = float((err / lim).max())
        assert ratio <= 1.0, (what, "largest error / bound", ratio)
        return ratio
    return 0.0


# ---- the inputs the CPU and the GPU tests share (made once per key, never changed) ----
_cache = {}


def noise_grid(dims):
    """(origin, spacing) of a grid over [-1.2, 1.2]^3 whose y axis runs backwards."""
    nx, ny, nz = dims
    return np.asarray([-1.2, 1.2, -1.2], F), np.asarray([2.4 / (nx - 1), -2.4 / (ny - 1), 2.4 / (nz - 1)], F)


def mixed_points(dims, o, sp, n):
    """n points: grid points, face points, points inside, points outside, NaN and inf points."""
    key = ("mixed", tuple(dims), n)
    if key not in _cache:
        rng = np.random.default_rng(n)
        top = (np.asarray(dims) - 1).astype(np.float64)
        kind = np.arange(n) % 8
        u = rng.uniform(0, 1, size=(n, 3)) * top
        grid = np.floor(rng.uniform(0, 1, size=(n, 3)) * (top + 1))
        u = np.where((kind == 0)[:, None], grid, u)
        face, axis, side = kind == 1, rng.integers(0, 3, n), rng.integers(0, 2, n)
        for c in range(3):
            u[:, c] = np.where(face & (axis == c), side * top[c], u[:, c])
        u = np.where((kind == 2)[:, None], rng.uniform(-0.5, 1.5, size=(n, 3)) * top, u)
        p = (o.astype(np.float64) + u * sp.astype(np.float64)).astype(F)
        p[kind == 0] = (o + grid[kind == 0].astype(F) * sp).astype(F)
        odd = np.asarray([np.nan, np.inf, -np.inf], F)
        rows = np.flatnonzero(kind == 3)
        p[rows, rng.integers(0, 3, len(rows))] = odd[rng.integers(0, 3, len(rows))]
        p.setflags(write=False)
        _cache[key] = p
    return _cache[key]


def noise_grads(n, seed=3):
    """(grad_value (n,), grad_gradient (n, 3)) uniform in (-1, 1)."""
    key = ("grads", n, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        gv, gg = rng.uniform(-1, 1, n).astype(F), rng.uniform(-1, 1, (n, 3)).astype(F)
        gv.setflags(write=False), gg.setflags(write=False)
        _cache[key] = (gv, gg)
    return _cache[key]


def noise_previous(dims, seed=5):
    """Non-zero noise as the previous content of grad_values, (nz, ny, nx)."""
    key = ("prev", tuple(dims), seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        a = (rng.uniform(0.25, 1.0, dims[::-1]) * rng.choice([-1.0, 1.0], dims[::-1])).astype(F)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def exact_family(dims, k=0, seed=0):
    """The family in which every product and every sum, in any order, is exact: f in eighths (both ends included), spacing
    (2^k, -2^k, 2^-k), grads integers in [-8, 8], previous content integers in [-8, 8], 64 points per cell divided by the number of cells
    that share an element.  Then every weight product is a multiple of 2^-9 and at most 1, every q a multiple of 2^-1 and at most 16 in
    size, every term and every contribution a multiple of 2^-9 of size at most 8 + 3 * 16 = 56, and every partial sum of an element a
    multiple of 2^-9 whose size is at most S = |a| + sum |c|.  The tests assert S < 2^12 on the data they use: 21 bits, under the 24 of
    float32.  -> (origin, spacing, points, grad_value, grad_gradient, previous)."""
    key = ("exact", tuple(dims), k, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * seed + 10 * (k + 1) + sum(dims))
        nx, ny, nz = dims
        o = np.asarray([-1.5, 2.25, 0.5], F)
        sp = np.asarray([2.0 ** k, -(2.0 ** k), 2.0 ** -k], F)
        sharing = min(2, nx - 1) * min(2, ny - 1) * min(2, nz - 1)  # the cells whose points can reach one element
        per_cell = 64 // sharing
        cells = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"), axis=-1).reshape(-1, 3)
        cells = np.repeat(cells, per_cell, axis=0)
        e = rng.integers(0, 9, cells.shape)  # eighths, both ends included
        u = cells + e / 8.0
        order = rng.permutation(len(u))
        p = (o.astype(np.float64) + u[order] * sp.astype(np.float64)).astype(F)
        n = len(p)
        gv = rng.integers(-8, 9, n).astype(F)
        gg = rng.integers(-8, 9, (n, 3)).astype(F)
        prev = rng.integers(-8, 9, (nz, ny, nx)).astype(F)
        for a in (o, sp, p, gv, gg, prev):
            a.setflags(write=False)
        _cache[key] = (o, sp, p, gv, gg, prev)
    return _cache[key]

"""The bitwise-reproducible form of the sampler's adjoint (include/cgrt.h cgrt_sample_grid_grad_repro*), restated in
numpy.  Not a test module; numpy only.

The contributions are grid_field_grad_ref.contributions, the float form's own; a contribution that compares equal to zero is not a
contribution (a NaN is one).  Per grid element with previous content a and contributions x_1..x_m (float32), n the call's point count:
    S    = min(24, 38 - bitlength(n))
    x_j  = +-M_j * 2^(e'_j - 150),  e'_j = max(exponent field, 1),  M_j the 24-bit significand (a subnormal has no implicit bit)
    E    = max e'_j,  d_j = E - e'_j
    T_j  = +-(M_j << (S - d_j)) if d_j <= S else +-(M_j >> (d_j - S))   (0 once the shift reaches 24)
    I    = sum T_j                       (int64: the only sum there is, and it is an integer sum)
    new  = fl32(fl64(a) + fl64(I) * 2^(E - 150 - S))
A non-finite contribution makes the element fl32(a + s): s NaN if a NaN or both infinities are present, else the infinity present.  Every
NaN result is the quiet NaN 0x7fc00000.  Elements without a contribution keep their bytes.  The integer terms are
surface_grad_repro_ref.terms, the surface form's, under the grid's S."""
import numpy as np

import grid_field_grad_ref as aref
from surface_grad_repro_ref import terms

F = np.float32
QNAN = np.uint32(0x7FC00000)


def shift(n):
    """S of a call with n points."""
    return min(24, 38 - int(n).bit_length())


def accumulate(a, dest, x, n):
    """The new content of the flat float32 array `a` after the contributions x (float32, none of them equal to zero) into elements dest
    of a call with n points.  Returns a new float32 array; a is not modified.  Elements no contribution names keep their bytes."""
    a = np.ascontiguousarray(a, F).reshape(-1)
    x = np.ascontiguousarray(x, F).reshape(-1)
    dest = np.asarray(dest, np.int64).reshape(-1)
    assert len(x) == len(dest)
    S = shift(n)
    b = x.view(np.uint32).astype(np.int64)
    ef = (b >> 23) & 0xFF
    finite = ef != 0xFF
    touched = np.zeros(len(a), bool)
    touched[dest] = True
    E = np.zeros(len(a), np.int64)
    np.maximum.at(E, dest[finite], np.maximum(ef[finite], 1))
    I = np.zeros(len(a), np.int64)
    np.add.at(I, dest[finite], terms(x[finite], E[dest[finite]], S))
    with np.errstate(over="ignore", invalid="ignore"):
        new = (a.astype(np.float64) + np.ldexp(I.astype(np.float64), (np.maximum(E, 1) - 150 - S).astype(np.int32))).astype(F)
        kinds = np.zeros((3, len(a)), bool)  # +inf, -inf, NaN
        frac = (b & 0x7FFFFF) != 0
        kinds[0, dest[~finite & ~frac & (b >> 31 == 0)]] = True
        kinds[1, dest[~finite & ~frac & (b >> 31 != 0)]] = True
        kinds[2, dest[~finite & frac]] = True
        any_kind = kinds.any(0)
        s = np.where(kinds[2] | (kinds[0] & kinds[1]), np.nan, np.where(kinds[0], np.inf, -np.inf)).astype(F)
        new = np.where(any_kind, a + s, new).astype(F)
    new = new.view(np.uint32).copy()
    new[np.isnan(new.view(F))] = QNAN
    return np.where(touched, new, a.view(np.uint32)).view(F)


_cache = {}


def pile_up(n, seed=7):
    """The most contended case there is: n points inside the one cell of a 2 x 2 x 2 grid (y spacing negative), grads whose sizes are
    spread over 40 binades (2^-20 .. 2^19) with both signs, non-zero previous content.  Made once per (n, seed) and read-only.
    -> (origin, spacing, dims, points, grad_value, grad_gradient, previous)."""
    key = (n, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        o, sp, dims = np.asarray([-1.0, 1.0, 0.5], F), np.asarray([2.0, -2.0, 0.25], F), (2, 2, 2)
        p = (o.astype(np.float64) + rng.uniform(0.0, 1.0, (n, 3)) * sp.astype(np.float64)).astype(F)
        gv = (rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
        gg = (rng.uniform(-1, 1, (n, 3)) * 2.0 ** rng.integers(-20, 20, (n, 3))).astype(F)
        prev = (np.arange(8, dtype=F) - F(3.5)).reshape(2, 2, 2)
        for a in (o, sp, p, gv, gg, prev):
            a.setflags(write=False)
        _cache[key] = (o, sp, dims, p, gv, gg, prev)
    return _cache[key]


def adjoint(origin, spacing, dims, points, grad_value=None, grad_gradient=None, clamp=False, previous=None, n=None):
    """The (nz, ny, nx) float32 volume after the reproducible call on n points (default: len(points)).  `previous` (float32, default
    zeros) is taken by its bytes: a signalling NaN or a -0 that no contribution names comes back as it went in."""
    nx, ny, nz = (int(x) for x in dims)
    inside, index, c = aref.contributions(origin, spacing, dims, points, grad_value, grad_gradient, clamp)
    prev = np.zeros((nz, ny, nx), F) if previous is None else np.ascontiguousarray(previous, F).reshape(nz, ny, nx)
    added = inside[:, None] & (c != 0)  # a NaN is not equal to 0 and is a contribution
    return accumulate(prev, index[added], c[added], len(inside) if n is None else n).reshape(nz, ny, nx)

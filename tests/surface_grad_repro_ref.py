"""The bitwise-reproducible form of the table adjoint (include/cgrt.h cgrt_interpolate_hits_grad_repro*, cgrt_surface_*_grad_repro_device;
DESIGN.md 5.28), restated in numpy.  Not a test module; numpy only.

Per table element with previous content a and contributions x_1..x_m (float32, each one rounded product w * g), n the call's item count:
    S    = min(24, 38 - bitlength(3 n))
    x_j  = +-M_j * 2^(e'_j - 150),  e'_j = max(exponent field, 1),  M_j the 24-bit significand (a subnormal has no implicit bit)
    E    = max e'_j,  d_j = E - e'_j
    T_j  = +-(M_j << (S - d_j)) if d_j <= S else +-(M_j >> (d_j - S))   (0 once the shift reaches 24)
    I    = sum T_j                       (int64: the only sum there is, and it is an integer sum)
    new  = fl32(fl64(a) + fl64(I) * 2^(E - 150 - S))
A non-finite contribution makes the element fl32(a + s): s NaN if a NaN or both infinities are present, else the infinity present.  Every
NaN result is the quiet NaN 0x7fc00000.  Elements without a contribution keep their bytes."""
import numpy as np

import surface_ref as sr

QNAN = np.uint32(0x7FC00000)


def shift(n):
    """S of a call with n items."""
    return min(24, 38 - (3 * int(n)).bit_length())


def terms(x, E, S):
    """The int64 terms T of the finite float32 contributions x under their elements' E (int64, one per contribution)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    ef = (b >> 23) & 0xFF
    M = (b & 0x7FFFFF) | np.where(ef > 0, 1 << 23, 0)
    d = np.asarray(E, np.int64) - np.maximum(ef, 1)
    assert (d >= 0).all()
    left = M << np.clip(S - d, 0, 24)
    right = np.where(d - S >= 24, 0, M >> np.clip(d - S, 0, 23))
    T = np.where(d <= S, left, right)
    return np.where(b >> 31 != 0, -T, T)


def accumulate(a, dest, x, n):
    """The new content of the flat float32 table `a` after the contributions x (float32) into elements dest (indices into a) of a call
    with n items.  Returns a new float32 array; a is not modified."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
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
        new = (a.astype(np.float64) + np.ldexp(I.astype(np.float64), (np.maximum(E, 1) - 150 - S).astype(np.int32))).astype(np.float32)
        kinds = np.zeros((3, len(a)), bool)  # +inf, -inf, NaN
        frac = (b & 0x7FFFFF) != 0
        kinds[0, dest[~finite & ~frac & (b >> 31 == 0)]] = True
        kinds[1, dest[~finite & ~frac & (b >> 31 != 0)]] = True
        kinds[2, dest[~finite & frac]] = True
        any_kind = kinds.any(0)
        s = np.where(kinds[2] | (kinds[0] & kinds[1]), np.nan, np.where(kinds[0], np.inf, -np.inf)).astype(np.float32)
        new = np.where(any_kind, a + s, new).astype(np.float32)
    new = new.view(np.uint32).copy()
    new[np.isnan(new.view(np.float32))] = QNAN
    return np.where(touched, new, a.view(np.uint32)).view(np.float32)


def contributions(sd, w, prim, hit, grad_out, channels):
    """(dest, x) of a call: every valid item's three rounded float32 products per channel and the flat table elements they go to, in
    item order.  grad_out (n, C) float32; its rows behind invalid items are never read."""
    g = np.asarray(grad_out, np.float32).reshape(-1, channels)
    ok = sr.triangle_mask(sd, hit, prim)
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[np.asarray(prim, np.int64)[ok]]
    wk, gk = np.asarray(w, np.float32)[ok], g[ok]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        x = wk[:, :, None] * gk[:, None, :]  # float32 times float32, each product rounded once
    dest = tri[:, :, None] * channels + np.arange(channels)[None, None, :]
    return dest.reshape(-1), x.astype(np.float32).reshape(-1)


def adjoint(sd, w, prim, hit, grad_out, init, n=None):
    """The (nverts, C) float32 table after the reproducible call on n items (default: len(grad_out)) with float32 weights w (n, 3)."""
    init = np.ascontiguousarray(init, np.float32)
    C = init.shape[1]
    g = np.asarray(grad_out, np.float32).reshape(-1, C)
    dest, x = contributions(sd, w, prim, hit, g, C)
    return accumulate(init, dest, x, len(g) if n is None else n).reshape(init.shape)

"""The adjoint of the surface-attribute mix with respect to the per-vertex table (include/cgrt.h cgrt_interpolate_hits_grad*,
cgrt_surface_*_grad_device), restated in float64 on top of surface_ref.weights.  Not a test module; numpy only.

For every (vertex, channel) the restatement gives
    ref  the initial value plus the sum of w * g over the element's contributions, in float64, from the float32 weights (a product of
         two float32 values is exact in float64);
    S    |initial| plus the sum of |w * g|;
    m    the number of contributions (the same for every channel of a vertex).
The device adds the m products, each rounded to float32, and the initial value in float32 in an order nobody fixes.  Any summation
order of m + 1 terms obeys Higham's bound for recursive summation, gamma(m) * S; one more u covers the rounding of each product:

    |got - ref| <= gamma(m + 1) * S + (m + 1) * 2^-126,   gamma(k) = k * u / (1 - k * u),  u = 2^-24

The absolute term allows every product and partial sum to lose a denormal's worth; the tests keep |values| in [2^-10, 2^10], where it
never decides.  The bound is the check only where m <= M_CAP = 512: losing one add of average size then moves the element by S / 512 or
more, against about 3e-5 * S allowed."""
import numpy as np

import surface_ref as sr

U = 2.0 ** -24
M_CAP = 512


def adjoint(sd, w, prim, hit, grad_out, init=None):
    """(ref, S, m): float64 (nverts, C), float64 (nverts, C), int64 (nverts,) for the items' float32 weights w (n, 3), their prim / hit
    columns and grad_out (n, C); init (nverts, C) is the table's content before the call (zeros when None).  grad_out of an invalid
    item is never read."""
    g = np.asarray(grad_out, np.float32)
    g = g.reshape(len(g), -1)
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    init = np.zeros((nverts, g.shape[1]), np.float64) if init is None else np.asarray(init, np.float32).astype(np.float64).reshape(nverts, g.shape[1])
    ref, S, m = init.copy(), np.abs(init), np.zeros(nverts, np.int64)
    ok = sr.triangle_mask(sd, hit, prim)
    if ok.any():
        tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[np.asarray(prim, np.int64)[ok]]
        wk, gk = np.asarray(w, np.float32)[ok].astype(np.float64), g[ok].astype(np.float64)
        for k in range(3):
            p = wk[:, k : k + 1] * gk
            np.add.at(ref, tri[:, k], p)
            np.add.at(S, tri[:, k], np.abs(p))
            np.add.at(m, tri[:, k], 1)
    return ref, S, m


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def bound(S, m):
    """The largest |got - ref| any order of the additions allows, per element ((nverts, C))."""
    m = np.asarray(m, np.float64)[:, None]
    return gamma(m + 1.0) * S + (m + 1.0) * 2.0 ** -126


def check(got, ref, S, m, what=""):
    """Assert that `got` (float32 (nverts, C)) is finite and within the bound of `ref` wherever m <= M_CAP; returns (elements beyond the
    cap, touched elements).  The figures are printed before anything is asserted."""
    got = np.asarray(got, np.float32).astype(np.float64).reshape(ref.shape)
    capped = np.broadcast_to((m <= M_CAP)[:, None], ref.shape)
    err, lim = np.abs(got - ref), bound(S, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lim > 0, err / lim, 0.0)
    touched = int((m > 0).sum()) * ref.shape[1]
    beyond = int((m > M_CAP).sum()) * ref.shape[1]
    worst = float(np.nanmax(np.where(capped, ratio, 0.0))) if ref.size else 0.0
    print(f"{what}: touched {touched} beyond-cap {beyond} max m {int(m.max()) if len(m) else 0} worst err/bound {worst:.3g}")
    assert np.isfinite(got).all(), (what, "not finite")
    bad = capped & ~(err <= lim)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), err[bad][:3], lim[bad][:3])
    return beyond, touched

"""The definition of the signed-distance / occupancy queries (include/cgrt.h "Signed distance and occupancy") on the CPU,
written from that text: dist2 from closest_ref.brute, the crossing counts from crossings_ref.all_pairs (the oracle's
intersectRayWithTriangle on the unbounded ray from the point), the majority vote over the parities, np.sqrt in float32, the sign, and the
rule for non-finite points and scenes without meshes.  Beside it the grid-point formula in float32."""
import numpy as np

import closest_ref as cr
import crossings_ref as xr

F32 = np.float32


def parity_votes(orc, sd, points, directions):
    """(n,) number of directions along which the unbounded ray from the point crosses an odd number of triangles."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    votes = np.zeros(len(p), np.int64)
    for d in np.asarray(directions, np.float32).reshape(-1, 3):
        rays = np.zeros((len(p), 7), np.float32)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = p, d, np.inf
        hit, _ = xr.all_pairs(orc, sd, rays)
        votes += hit.sum(axis=1) & 1
    return votes


def reference(orc, sd, points, directions, max_dist2=np.inf):
    """(sdf (n,) float32, inside (n,) bool) of every point by the definition."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    dirs = np.asarray(directions, np.float32).reshape(-1, 3)
    assert len(dirs) % 2 == 1
    sdf = np.full(len(p), np.inf, np.float32)
    inside = np.zeros(len(p), bool)
    finite = np.isfinite(p).all(axis=1)
    T = int(np.asarray(sd.tri).reshape(-1, 3).shape[0])
    if T == 0 or not finite.any():
        return sdf, inside
    q = p[finite]
    with np.errstate(all="ignore"):
        s = np.sqrt(cr.brute(sd, q, max_dist2)["dist2"])  # (float32 in, float32 out: correctly rounded; +inf stays +inf)
    assert s.dtype == np.float32
    ins = parity_votes(orc, sd, q, dirs) > len(dirs) // 2
    sdf[finite] = np.where(ins, -s, s)
    inside[finite] = ins
    return sdf, inside


def grid_points(origin, spacing, dims):
    """(nx * ny * nz, 3) float32: point (ix, iy, iz) = origin.c + float32(i_c) * spacing.c (the product rounded, then the sum) at row
    (iz * ny + iy) * nx + ix.  Written as plain loops over the indices."""
    o, sp = np.asarray(origin, np.float32).reshape(3), np.asarray(spacing, np.float32).reshape(3)
    nx, ny, nz = (int(x) for x in dims)
    out = np.zeros((nx * ny * nz, 3), np.float32)
    with np.errstate(all="ignore"):
        for iz in range(nz):
            for iy in range(ny):
                for ix in range(nx):
                    r = (iz * ny + iy) * nx + ix
                    for c, i in enumerate((ix, iy, iz)):
                        prod = F32(F32(i) * sp[c])
                        out[r, c] = F32(o[c] + prod)
    return out

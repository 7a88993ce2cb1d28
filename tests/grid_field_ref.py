"""The numpy restatement of include/cgrt.h "Grid fields": the trilinear sample with its gradient, the march of a ray with its
refinement, and the work counters of cgrt_debug_march_work.  float32 arrays throughout, so every operation rounds on its own, exactly as
the header orders them; vectorised over points and over rays (an active mask).  Every result is given as the bytes the library stores:
computed NaNs canonical (0x7fc00000), `outside` passed through bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32
CANON = np.uint32(0x7FC00000)
MISS, HIT, EXHAUSTED, NONFINITE = 0, 1, 2, 3
FIELD_CLAMP = 1
INSIDE_ABOVE = 1
HIT_DTYPE = np.dtype([("t", F), ("value", F), ("steps", np.uint32), ("status", np.uint32), ("gradient", F, 3), ("reserved", np.uint32)])


def canonical(a):
    """float32 array -> the stored words (uint32): every NaN is 0x7fc00000."""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), CANON, a.view(np.uint32))


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def cell(origin, spacing, dims, points, clamp=False):
    """(inside (n,) bool, i (n, 3) int64, f (n, 3) float32) of the header's steps; rows of outside points hold zeros."""
    o, sp = np.asarray(origin, F).reshape(3), np.asarray(spacing, F).reshape(3)
    n3 = np.asarray([int(x) for x in dims], np.int64)
    top = (n3 - 1).astype(F)
    p = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = (p - o[None, :]) / sp[None, :]
        if clamp:
            u = np.where(u < 0, F(0), np.where(u > top[None, :], top[None, :], u))
        inside = np.all((u >= 0) & (u <= top[None, :]), axis=1)
        us = np.where(inside[:, None], u, F(0))
        i = np.minimum(np.floor(us).astype(np.int64), (n3 - 2)[None, :])
        f = (us - i.astype(F)).astype(F)
    return inside, i, f


def sample(values, origin, spacing, points, outside=np.nan, clamp=False):
    """values (nz, ny, nx) float32 -> (value words (n,) uint32, gradient words (n, 3) uint32, inside (n,) uint8)."""
    v = np.ascontiguousarray(values, F)
    nz, ny, nx = v.shape
    sp = np.asarray(spacing, F).reshape(3)
    inside, i, f = cell(origin, spacing, (nx, ny, nz), points, clamp)
    flat = v.reshape(-1)
    base = (i[:, 2] * ny + i[:, 1]) * nx + i[:, 0]
    c = lambda x, y, z: flat[base + x + y * nx + z * nx * ny]  # noqa: E731
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(all="ignore"):
        d = {(y, z): c(1, y, z) - c(0, y, z) for y in (0, 1) for z in (0, 1)}
        a = {(y, z): c(0, y, z) + fx * d[y, z] for y in (0, 1) for z in (0, 1)}
        e = {z: a[1, z] - a[0, z] for z in (0, 1)}
        b = {z: a[0, z] + fy * e[z] for z in (0, 1)}
        w = b[1] - b[0]
        value = b[0] + fz * w
        lerp = lambda p, q, t: p + t * (q - p)  # noqa: E731
        gz = w / sp[2]
        gy = lerp(e[0], e[1], fz) / sp[1]
        gx = lerp(lerp(d[0, 0], d[1, 0], fy), lerp(d[0, 1], d[1, 1], fy), fz) / sp[0]
    assert value.dtype == F and gx.dtype == F and gy.dtype == F and gz.dtype == F
    out_bits = np.asarray(outside, F).reshape(1).view(np.uint32)[0]
    vw = np.where(inside, canonical(value), out_bits)
    gw = np.where(inside[:, None], canonical(np.stack([gx, gy, gz], axis=1)), np.uint32(0))
    return vw.astype(np.uint32), gw.astype(np.uint32), inside.astype(np.uint8)


def sample_f(values, origin, spacing, points, outside=np.nan, clamp=False):
    """sample as float32 arrays (value, gradient, inside bool)."""
    vw, gw, ins = sample(values, origin, spacing, points, outside, clamp)
    return vw.view(F), gw.view(F), ins.astype(bool)


def _as_rays(rays):
    r = np.asarray(rays)
    if r.dtype.fields is not None:
        r = np.ascontiguousarray(r).view(F).reshape(-1, 7)
    return np.ascontiguousarray(r, F).reshape(-1, 7)


def march(values, origin, spacing, rays, iso=0.0, relax=1.0, min_step=1e-4, hit_eps=1e-4, max_steps=256, refine=0, inside_above=False):
    """-> (records (n,) HIT_DTYPE with canonical NaNs, work (entered, main-loop samples, refinement samples))."""
    v = np.ascontiguousarray(values, F)
    nz, ny, nx = v.shape
    o3, sp = np.asarray(origin, F).reshape(3), np.asarray(spacing, F).reshape(3)
    top = np.asarray([nx - 1, ny - 1, nz - 1], F)
    iso, relax, min_step, hit_eps = F(iso), F(relax), F(min_step), F(hit_eps)
    r = _as_rays(rays)
    n = len(r)
    o, d, t_ray = r[:, 0:3], r[:, 3:6], r[:, 6]
    t_out = np.full(n, np.inf, F)
    v_out = np.zeros(n, F)
    steps = np.zeros(n, np.uint32)
    status = np.full(n, MISS, np.uint32)
    grad = np.zeros((n, 3), np.uint32)
    work = [0, 0, 0]

    def value_at(idx, t):
        with np.errstate(all="ignore"):
            p = o[idx] + t[:, None] * d[idx]
        return sample(v, o3, sp, p, outside=np.nan, clamp=True)

    def gap(val):
        with np.errstate(all="ignore"):
            return (iso - val) if inside_above else (val - iso)

    with np.errstate(all="ignore"):
        length = np.sqrt(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]))
        ok = np.all(np.isfinite(o), axis=1) & np.all(np.isfinite(d), axis=1) & ~np.isnan(t_ray) & (length > 0) & np.isfinite(length)
        t0 = np.zeros(n, F)
        t1 = t_ray.copy()
        for c in range(3):
            far = o3[c] + top[c] * sp[c]
            lo, hi = (o3[c] if o3[c] < far else far), (o3[c] if o3[c] > far else far)
            zero = d[:, c] == 0
            ok &= ~(zero & ~((lo <= o[:, c]) & (o[:, c] <= hi)))
            ta, tb = (lo - o[:, c]) / d[:, c], (hi - o[:, c]) / d[:, c]
            t0 = np.where(zero, t0, _max(t0, _min(ta, tb)))
            t1 = np.where(zero, t1, _min(t1, _max(ta, tb)))
        ok &= t0 <= t1
    work[0] = int(ok.sum())
    act = np.flatnonzero(ok)  # the rays still marching
    t = t0[act].astype(F)
    t_prev = np.zeros(len(act), F)
    have_prev = np.zeros(len(act), bool)
    k = 0
    hit_idx, hit_ta, hit_tb, hit_prev = [], [], [], []
    while len(act):
        vw, _, _ = value_at(act, t)
        val = vw.view(F)
        work[1] += len(act)
        g = gap(val)
        nonfin = np.isnan(g)
        hit = ~nonfin & (g <= hit_eps)
        miss = ~nonfin & ~hit & (t >= t1[act])
        exh = ~nonfin & ~hit & ~miss & (k + 1 == max_steps)
        a = act[nonfin]
        t_out[a], v_out[a], steps[a], status[a] = t[nonfin], np.nan, k, NONFINITE
        a = act[miss]
        steps[a] = k
        a = act[exh]
        t_out[a], v_out[a], steps[a], status[a] = t[exh], val[exh], max_steps, EXHAUSTED
        a = act[hit]
        steps[a], status[a] = k, HIT
        hit_idx.append(a), hit_ta.append(t_prev[hit]), hit_tb.append(t[hit]), hit_prev.append(have_prev[hit])
        go = ~(nonfin | hit | miss | exh)
        act, t, g = act[go], t[go], g[go]
        with np.errstate(all="ignore"):
            dt = _max((relax * g) / length[act], min_step)
            t_prev, t = t, _min(t + dt, t1[act])
        have_prev = np.ones(len(act), bool)
        k += 1
    if hit_idx:
        idx, ta, tb, prev = (np.concatenate(x) for x in (hit_idx, hit_ta, hit_tb, hit_prev))
        ta, tb = ta.astype(F), tb.astype(F)
        for _ in range(int(refine)):
            if not prev.any():
                break
            with np.errstate(all="ignore"):
                tm = ta[prev] + F(0.5) * (tb[prev] - ta[prev])
            vw, _, _ = value_at(idx[prev], tm)
            work[2] += int(prev.sum())
            with np.errstate(all="ignore"):
                below = gap(vw.view(F)) <= hit_eps
            nb, na = tb[prev], ta[prev]
            nb[below], na[~below] = tm[below], tm[~below]
            tb[prev], ta[prev] = nb, na
        vw, gw, _ = value_at(idx, tb)
        t_out[idx], v_out[idx] = tb, vw.view(F)
        grad[idx] = gw
    rec = np.zeros(n, HIT_DTYPE)
    rec["t"] = canonical(t_out).view(F)
    rec["value"] = canonical(v_out).view(F)
    rec["steps"], rec["status"] = steps, status
    rec["gradient"] = grad.view(F)
    return rec, tuple(work)

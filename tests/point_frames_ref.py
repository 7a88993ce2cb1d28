"""Point-set frames (include/cgrt.h "Point-set frames") restated in numpy from their definition -- not from the library's
sources.  Not a test module; numpy only.  The slots come from tests/point_neighbors_ref.py; steps 2 to 7 are float32 arithmetic vectorised
over the queries, every operation rounded on its own (numpy does not contract), one numpy operation per fl() of the definition.

  * frames(): the (n,) FRAME records and the (n, k) neighbour slots; with detail=True also what the tests of the definition itself look at
    (sweeps run, the off-diagonals at the loop's end, the float32 covariance, the smallest and largest scale-carrying product or quotient);
  * truth(): numpy.linalg.eigh in float64 on the float64 covariance of the same neighbours, an independent computation."""
import numpy as np

import point_neighbors_ref as nref

F32 = np.float32
NO_PRIM = nref.NO_PRIM
SWEEPS = 8
CANONICAL_NAN = 0x7FC00000
FRAME = np.dtype([("centroid", F32, 3), ("used", np.uint32), ("normal", F32, 3), ("lambda0", F32), ("tangent_u", F32, 3), ("lambda1", F32),
                  ("tangent_v", F32, 3), ("lambda2", F32)])
assert FRAME.itemsize == 64
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
ONE, TWO = F32(1), F32(2)


class _Range:
    """The smallest non-zero and the largest magnitude, per query, of the values it is shown (rows where `on` is false are not looked at)."""

    def __init__(self, n):
        self.lo, self.hi = np.full(n, np.inf), np.zeros(n)

    def see(self, on, *values):
        for v in values:
            a = np.abs(v.astype(np.float64))
            a = np.where(np.isnan(a), np.inf, a)
            self.hi = np.where(on, np.maximum(self.hi, a), self.hi)
            self.lo = np.where(on & (a > 0), np.minimum(self.lo, a), self.lo)


def _rotate(on, A, p, q, r, V, rng):
    """Step 4's rotation in the plane (p, q) for the queries `on`; A: dict of the six entries keyed by sorted index pairs, V: columns."""
    key = lambda i, j: (min(i, j), max(i, j))  # noqa: E731
    app, aqq, apq, arp, arq = A[(p, p)], A[(q, q)], A[key(p, q)], A[key(r, p)], A[key(r, q)]
    on = on & (apq != 0)
    theta = (aqq - app) / (TWO * apq)
    t = np.where(theta < 0, -ONE, ONE) / (np.abs(theta) + np.sqrt(theta * theta + ONE))
    c = ONE / np.sqrt(t * t + ONE)
    s = t * c
    h = t * apq
    ca, sa, sb, cb = c * arp, s * arq, s * arp, c * arq
    rng.see(on, h, ca, sa, sb, cb)
    A[(p, p)] = np.where(on, app - h, app)
    A[(q, q)] = np.where(on, aqq + h, aqq)
    A[key(p, q)] = np.where(on, F32(0), apq)
    A[key(r, p)] = np.where(on, ca - sa, arp)
    A[key(r, q)] = np.where(on, sb + cb, arq)
    vp, vq = V[p], V[q]
    V[p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
    V[q] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)


def _exchange(d, V, a, b):
    """Step 5: d_b < d_a -> the two eigenvalues and their columns change places."""
    sw = d[b] < d[a]
    d[a], d[b] = np.where(sw, d[b], d[a]), np.where(sw, d[a], d[b])
    V[a], V[b] = np.where(sw[:, None], V[b], V[a]), np.where(sw[:, None], V[a], V[b])


def _lead_sign(v):
    """Step 6: negated iff the component of largest magnitude (the first on a tie; a NaN never) is < 0."""
    best, pick = np.abs(v[:, 0]), v[:, 0]
    m = np.abs(v[:, 1]) > best
    best, pick = np.where(m, np.abs(v[:, 1]), best), np.where(m, v[:, 1], pick)
    pick = np.where(np.abs(v[:, 2]) > best, v[:, 2], pick)
    return np.where((pick < 0)[:, None], -v, v)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def solve(cov6, orient=None, rng=None):
    """Steps 4 to 6 on (n, 6) float32 matrices {xx, xy, xz, yy, yz, zz}: (eigenvalues (n, 3), normal, tangent_u, tangent_v (n, 3) each,
    sweeps run (n,), the off-diagonals at the loop's end (n, 3))."""
    a = np.asarray(cov6, F32).reshape(-1, 6)
    n = len(a)
    rng = rng or _Range(n)
    with np.errstate(**_ERR):
        A = {(0, 0): a[:, 0].copy(), (0, 1): a[:, 1].copy(), (0, 2): a[:, 2].copy(), (1, 1): a[:, 3].copy(), (1, 2): a[:, 4].copy(),
             (2, 2): a[:, 5].copy()}
        V = [np.tile(np.eye(3, dtype=F32)[:, c], (n, 1)) for c in range(3)]  # V[c]: column c, (n, 3) over the rows i
        on = np.ones(n, bool)
        sweeps = np.zeros(n, np.int32)
        for _ in range(SWEEPS):
            _rotate(on, A, 0, 1, 2, V, rng)
            _rotate(on, A, 0, 2, 1, V, rng)
            _rotate(on, A, 1, 2, 0, V, rng)
            sweeps += on
            on = on & ~((A[(0, 1)] == 0) & (A[(0, 2)] == 0) & (A[(1, 2)] == 0))
        off = np.stack([A[(0, 1)], A[(0, 2)], A[(1, 2)]], 1)
        d = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
        _exchange(d, V, 0, 1)
        _exchange(d, V, 1, 2)
        _exchange(d, V, 0, 1)
        nrm, tu, tv = _lead_sign(V[0]), _lead_sign(V[1]), V[2]
        if orient is not None:
            o = np.asarray(orient, F32).reshape(-1, 3)
            assert len(o) == n
            flip = np.isfinite(o).all(1) & (_dot(nrm, o) < 0)
            nrm = np.where(flip[:, None], -nrm, nrm)
        w = np.stack([nrm[:, 1] * tu[:, 2] - nrm[:, 2] * tu[:, 1], nrm[:, 2] * tu[:, 0] - nrm[:, 0] * tu[:, 2],
                      nrm[:, 0] * tu[:, 1] - nrm[:, 1] * tu[:, 0]], 1)
        tv = np.where((_dot(w, tv) < 0)[:, None], -tv, tv)
    for x in (*d, nrm, tu, tv, off):
        assert x.dtype == F32
    return np.stack(d, 1), nrm, tu, tv, sweeps, off


def _canonical(x):
    """Step 7: every NaN as 0x7fc00000."""
    x = np.ascontiguousarray(x, F32).copy()
    x.view(np.uint32)[np.isnan(x)] = CANONICAL_NAN
    return x


def moments(slots, data):
    """Steps 2 and 3 on (n, k) neighbour slots: (used (n,), centroid (n, 3), covariance (n, 6), the scale-carrying ranges: of s / used --
    linear in the scale -- and of the products and quotients of step 3 -- quadratic)."""
    d = np.asarray(data, F32).reshape(-1, 3)
    n, k = slots.shape
    real = slots["index"] != NO_PRIM
    used = real.sum(1).astype(np.uint32)
    assert (real == (np.arange(k)[None, :] < used[:, None])).all(), "the real records of a slot come first"
    P = d[np.where(real, slots["index"], 0)] if len(d) else np.zeros((n, k, 3), F32)
    lin, quad = _Range(n), _Range(n)
    with np.errstate(**_ERR):
        ref = P[:, 0] if k else np.zeros((n, 3), F32)
        s = np.zeros((n, 3), F32)
        for j in range(k):
            s = np.where(real[:, j, None], s + (P[:, j] - ref), s)
        fu = used.astype(F32)
        mean = s / fu[:, None]
        c = ref + mean
        sums = np.zeros((n, 6), F32)
        for j in range(k):
            e = P[:, j] - c
            prod = np.stack([e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1], e[:, 1] * e[:, 2], e[:, 2] * e[:, 2]], 1)
            quad.see(real[:, j], *prod.T)
            sums = np.where(real[:, j, None], sums + prod, sums)
        cov = sums / fu[:, None]
    on = used > 0
    lin.see(on, *mean.T)
    quad.see(on, *cov.T)
    assert c.dtype == F32 and cov.dtype == F32
    return used, c, cov, lin, quad


def frames(points, data, k, radius2=None, max_dist2=np.inf, skip_same_index=False, orient=None, slots=None, detail=False):
    """(records (n,) FRAME, slots (n, k) RECORD); with detail=True a third value, a dict: 'sweeps' (n,), 'off' (n, 3) the off-diagonals at
    the loop's end, 'cov' (n, 6) float32, 'lin' = (lo, hi) and 'quad' = (lo, hi): the smallest non-zero and the largest magnitude of the
    scale-carrying products and quotients (float64; lo = inf where there is none)."""
    q = np.asarray(points, F32).reshape(-1, 3)
    n = len(q)
    if slots is None:
        slots = nref.neighbors(q, data, radius2, max_dist2, skip_same_index, k=k)[0] if n else np.zeros((0, k), nref.RECORD)
    used, c, cov, lin, quad = moments(slots, data)
    lam, nrm, tu, tv, sweeps, off = solve(cov, orient, quad)
    out = np.zeros(n, FRAME)
    out["centroid"], out["used"] = _canonical(c), used
    out["normal"], out["tangent_u"], out["tangent_v"] = _canonical(nrm), _canonical(tu), _canonical(tv)
    lam = _canonical(lam)
    out["lambda0"], out["lambda1"], out["lambda2"] = lam[:, 0], lam[:, 1], lam[:, 2]
    out[used == 0] = np.zeros((), FRAME)
    if not detail:
        return out, slots
    return out, slots, dict(sweeps=np.where(used > 0, sweeps, 0), off=off, cov=cov, lin=(lin.lo, lin.hi), quad=(quad.lo, quad.hi))


def truth(slots, data):
    """float64: (eigenvalues (n, 3) ascending, eigenvectors (n, 3, 3) as columns, trace (n,), max |p|^2 (n,)) of the covariance of each
    slot's real records about their float64 mean; rows with used == 0 are zeros."""
    d = np.asarray(data, np.float64).reshape(-1, 3)
    n, k = slots.shape
    lam, vec, tr, p2 = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros(n), np.zeros(n)
    for i in range(n):
        idx = slots["index"][i]
        idx = idx[idx != NO_PRIM]
        if len(idx) == 0:
            continue
        P = d[idx]
        e = P - P.mean(0)
        C = e.T @ e / len(idx)
        lam[i], vec[i] = np.linalg.eigh(C)
        tr[i], p2[i] = np.trace(C), (P * P).max()
    return lam, vec, tr, p2


def cloud(name, m=2000, n=300, seed=5):
    """The seeded test clouds: (data (m, 3), separate queries (n, 3)), float32.
    shell: a unit sphere shell with 1 % radial noise; patch: the plane z = 0.5 over the unit square, every eighth point a duplicate of
    another; offset: a cube of edge 0.01 at (100, 100, 100); cube: the uniform unit cube; holes: cube with NaN and inf rows."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    if name == "shell":
        v = rng.normal(size=(m + n, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True) * (1.0 + 0.01 * rng.normal(size=(m + n, 1)))
    elif name == "patch":
        p = np.concatenate([rng.random((m + n, 2)), np.full((m + n, 1), 0.5)], 1)
        p[7:m:8] = p[3:m:8][: len(p[7:m:8])]
        p[m:, 2] += 0.05 * rng.normal(size=n)  # (the queries hover about the plane)
    elif name == "offset":
        p = 100.0 + 0.01 * rng.random((m + n, 3))
    elif name in ("cube", "holes"):
        p = rng.random((m + n, 3))
        if name == "holes":
            p[5:m:11, 0], p[6:m:13, 1], p[9:m:17, 2] = np.nan, np.inf, -np.inf
            p[m + 3 :: 29, 1], p[m + 4 :: 31, 2] = np.nan, np.inf
    else:
        raise KeyError(name)
    p = p.astype(F32)
    return p[:m].copy(), p[m:].copy()


#: the across-scale cases: s -> the binary exponent of the base cloud's edge.  The late sweeps leave values down to about 2^-140 of the
#: trace T (about 2^-7 of the squared edge for 8 neighbours of 1200 points), and sums of squares reach 8 T: the envelope wants T and
#: T 2^2s within about [2^14, 2^120], so each s has a base cloud of its own.
SCALE_CASES = {-40: 52, -8: 32, 8: 32, 40: 12}


def scale_case(s, m=1200, n=300):
    """(data (m, 3), queries: its first n points) at scale 1 of the across-scale case s: the uniform unit cube times 2^SCALE_CASES[s]."""
    base = np.ldexp(np.random.default_rng(31).random((m, 3)).astype(F32), SCALE_CASES[s])
    return base, base[:n].copy()


def in_frame_envelope(detail, s):
    """(n,) bool: every scale-carrying product or quotient of the query is zero or a normal float at scale 1 and at 2^s (include/cgrt.h
    "Point-set frames", Scale)."""
    fmin, fmax = float(np.finfo(F32).tiny), float(np.finfo(F32).max)
    ok = np.ones(len(detail["sweeps"]), bool)
    for (lo, hi), f in ((detail["lin"], 2.0 ** s), (detail["quad"], 4.0 ** s)):
        ok &= (lo >= fmin) & (hi <= fmax) & (lo * f >= fmin) & (hi * f <= fmax)
    return ok

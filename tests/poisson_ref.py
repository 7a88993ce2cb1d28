"""Poisson-disk sets (include/cgrt.h "Poisson-disk sets") restated in numpy from their definition -- not from the
library's sources.  Not a test module; numpy only.  The dense forms serve up to a few thousand points (an all-pairs matrix, MAX_N); the
sparse forms a few hundred thousand.

  * the order words: word 3 of the Philox of sampling_ref.py, or the caller's priority; the order by np.lexsort over (index, P);
  * the all-pairs float32 d2 matrix, every subtraction, product and sum rounded on its own (numpy float32 arithmetic does not contract);
  * greedy(): the sequential pass of the definition;
  * rounds(): the synchronous-round form -- every undecided point looks at the states as the round found them -- and its round count;
  * conflict_pairs(), greedy_sparse(): the same conflicts and the same pass without the matrix -- candidates by binning into float64
    cells, the definition's float32 d2 on the candidates, the pass over the CSR of the pairs."""
import numpy as np

import sampling_ref as sref

F32 = np.float32
U64 = np.uint64
MAX_N = 8192
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def order_words(n, seed=0, priority=None):
    """(n,) uint64 holding the 32-bit words P_i."""
    if priority is not None:
        p = np.asarray(priority).astype(U64)
        assert p.shape == (n,) and (p <= U64(0xFFFFFFFF)).all()
        return p
    i = np.arange(n, dtype=U64)
    seed = int(seed)
    return sref.philox4x32_10([i & sref.MASK, i >> sref.S32, 0, 0], [seed & 0xFFFFFFFF, seed >> 32])[3]


def keys(n, seed=0, priority=None):
    """(P_i, i) as one Python-exact uint64 key per point: P_i * 2^32 + i."""
    return (order_words(n, seed, priority) << U64(32)) | np.arange(n, dtype=U64)


def finite(points):
    return np.isfinite(np.asarray(points, F32).reshape(-1, 3)).all(1)


def d2_matrix(points):
    """(n, n) float32: fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) with dx = fl(x_i - x_j)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    assert len(p) <= MAX_N
    with np.errstate(**_ERR):
        d = [p[:, None, k] - p[None, :, k] for k in range(3)]
        assert all(x.dtype == F32 for x in d)
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def conflicts(points, min_dist2, d2=None):
    """(n, n) bool: both finite, i != j, d2 < min_dist2 (NaN or <= 0: none)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    d2 = d2_matrix(p) if d2 is None else d2
    m = F32(min_dist2)
    assert not np.isposinf(m)
    with np.errstate(**_ERR):
        c = d2 < m if m > 0 else np.zeros(d2.shape, bool)
    f = finite(p)
    c = c & f[:, None] & f[None, :]
    np.fill_diagonal(c, False)
    return c


def greedy(points, min_dist2, seed=0, priority=None, d2=None):
    """(n,) bool: the sequential pass."""
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    c, f = conflicts(p, min_dist2, d2), finite(p)
    keep = np.zeros(n, bool)
    for i in np.argsort(keys(n, seed, priority), kind="stable"):
        if f[i] and not (c[i] & keep).any():
            keep[i] = True
    return keep


def conflict_pairs(points, min_dist2):
    """(c, 2) int64, every conflicting pair i < j once, in lexicographic order: conflicts()' upper triangle without the matrix.
    Candidates come from float64 cells of edge 1.001 * sqrt(min_dist2) (raised to extent * 2^-20 where the cloud is wider than 2^20
    such cells): d2 < min_dist2 implies fl(dx)^2 < min_dist2 (adding non-negative terms never decreases a rounded sum), so |dx| <
    sqrt(min_dist2) * (1 + 2^-24) per axis, a thousandth above which the edge lies: the two cells differ by at most one per axis.  Each
    of the 27 shifts of a point's cell is looked up in the sorted cell keys with searchsorted; the definition's float32 d2 decides."""
    p = np.asarray(points, F32).reshape(-1, 3)
    m = F32(min_dist2)
    assert not np.isposinf(m)
    none = np.zeros((0, 2), np.int64)
    idx = np.flatnonzero(finite(p))
    if not m > 0 or len(idx) < 2:
        return none
    q = p[idx].astype(np.float64)
    lo = q.min(0)
    edge = max(np.sqrt(float(m)) * 1.001, float((q.max(0) - lo).max()) * 2.0 ** -20)
    S = np.int64(1) << 21
    c = np.floor((q - lo) / edge).astype(np.int64) + 1  # 1 .. 2^20 + 1: a shift by -1 stays non-negative
    key = (c[:, 0] * S + c[:, 1]) * S + c[:, 2]
    order = np.argsort(key, kind="stable")
    skey, sidx = key[order], idx[order]
    out = []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                want = key + ((sx * S + sy) * S + sz)
                b, e = np.searchsorted(skey, want, "left"), np.searchsorted(skey, want, "right")
                cnt = e - b
                i = np.repeat(idx, cnt)
                j = sidx[np.repeat(b - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))]
                keep = i < j
                i, j = i[keep], j[keep]
                with np.errstate(**_ERR):
                    d = [p[i, k] - p[j, k] for k in range(3)]
                    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    assert d2.dtype == F32
                    hit = d2 < m
                out.append(np.stack([i[hit], j[hit]], 1))
    pairs = np.concatenate(out) if out else none
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def greedy_sparse(points, min_dist2, seed=0, priority=None, pairs=None):
    """(n,) bool: greedy()'s sequential pass in key order over the CSR of conflict_pairs() (`pairs`: its result, where the caller has it)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    pairs = conflict_pairs(p, min_dist2) if pairs is None else pairs
    a = np.concatenate([pairs[:, 0], pairs[:, 1]])
    b = np.concatenate([pairs[:, 1], pairs[:, 0]])
    adj = b[np.argsort(a, kind="stable")]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=off[1:])
    keep = np.zeros(n, bool)
    f = finite(p)
    off_l = off.tolist()
    for i in np.argsort(keys(n, seed, priority), kind="stable").tolist():
        if f[i] and not keep[adj[off_l[i] : off_l[i + 1]]].any():
            keep[i] = True
    return keep


def rounds(points, min_dist2, seed=0, priority=None, d2=None):
    """((n,) bool, the number of rounds): in a round every undecided point with a KEPT earlier conflicting point is rejected, every one
    whose earlier conflicting points are all rejected is kept, on the states as they were when the round began."""
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    k = keys(n, seed, priority)
    earlier = conflicts(p, min_dist2, d2) & (k[None, :] < k[:, None])  # [i, j]: j conflicts with i and comes before it
    UND, KEPT, REJ = 0, 1, 2
    state = np.where(finite(p), UND, REJ)
    count = 0
    while (state == UND).any():
        count += 1
        und = state == UND
        kept_before = (earlier & (state == KEPT)[None, :]).any(1)
        und_before = (earlier & und[None, :]).any(1)
        state = np.where(und & kept_before, REJ, np.where(und & ~und_before, KEPT, state))
        assert count <= n
    return state == KEPT, count


def check_set(points, min_dist2, keep, seed=0, priority=None, d2=None):
    """The defining properties: kept points are finite and pairwise free of conflicts; every finite point that is not kept conflicts with a
    kept point before it."""
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    keep = np.asarray(keep, bool)
    c, f, k = conflicts(p, min_dist2, d2), finite(p), keys(n, seed, priority)
    assert not (keep & ~f).any(), "a non-finite point is kept"
    assert not (c & keep[:, None] & keep[None, :]).any(), "two kept points conflict"
    covered = (c & keep[None, :] & (k[None, :] < k[:, None])).any(1)
    assert (covered | keep | ~f).all(), "a finite point is neither kept nor covered by an earlier kept point"


def line_case():
    """512 points on a line at spacing 0.6, priority = index, min_dist2 = 1: the even indices, 512 synchronous rounds."""
    p = np.zeros((512, 3), F32)
    p[:, 0] = (np.arange(512) * 0.6).astype(F32)
    return p, F32(1.0), np.arange(512, dtype=np.uint32)


def lattice_case():
    """An 8^3 lattice of spacing 0.25 (every coordinate and every distance exact)."""
    g = np.arange(8, dtype=F32) * F32(0.25)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)

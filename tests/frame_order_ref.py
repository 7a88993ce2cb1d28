"""The order builder's policy and the validity predicate of an order table, stated in NumPy (k_build_frame_order in trace_kernels.hip,
order_table_valid in capi_primary.cpp).  A helper module of test_frame_order_cpu.py and test_frame_order_gpu.py.

A launch has one POSITION per rank-local super-tile, padded to a multiple of 8; position p belongs to lane p % 8 (one XCD).  From the
longest wave time of every super-tile in a profile frame (`ticks`, 10 ns each), per lane:
  * the positions with ticks >= LIVE_TICKS are live, every other position (the padded ones included) keeps its own super-tile;
  * the live super-tiles are dealt to the live positions, in ascending order of position, by descending ticks, ties by position.
"""
import numpy as np

LIVE_TICKS = 500  # 5 us


def padded(n: int) -> int:
    return (n + 7) // 8 * 8


def build_order(ticks, live: int = LIVE_TICKS) -> np.ndarray:
    t = np.asarray(ticks, np.uint32)
    n = len(t)
    out = np.arange(padded(n), dtype=np.uint16)
    for lane in range(8):
        pos = np.arange(lane, n, 8)
        live_pos = pos[t[pos] >= live]  # ascending
        # descending ticks, ties by position: a stable sort of the negated ticks over positions that are already ascending
        by_ticks = live_pos[np.argsort(-t[live_pos].astype(np.int64), kind="stable")]
        out[live_pos] = by_ticks
    return out


def is_valid_order(table, nst: int) -> bool:
    """A permutation of the padded(nst) positions that keeps every position's % 8 residue and maps the padded positions to themselves."""
    t = np.asarray(table)
    n = padded(nst)
    if t.ndim != 1 or len(t) != n or not np.issubdtype(t.dtype, np.integer):
        return False
    t = t.astype(np.int64)
    p = np.arange(n)
    if (t < 0).any() or (t >= n).any() or len(np.unique(t)) != n:
        return False
    if ((t & 7) != (p & 7)).any():
        return False
    return bool((t[nst:] == p[nst:]).all())


def super_tiles(W: int, H: int, rect=None, rank: int = 0, nranks: int = 1) -> int:
    """Rank-local super-tiles (64x64 pixels) of a frame shape: make_frame's nst_rank."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    tx, ty = (x1 - x0 + 7) // 8, (y1 - y0 + 7) // 8
    nst = ((tx + 7) // 8) * ((ty + 7) // 8)
    return (nst + nranks - 1 - rank) // nranks


def reversal(nst: int) -> np.ndarray:
    """Every lane's real positions in reverse."""
    out = np.arange(padded(nst), dtype=np.uint16)
    for lane in range(8):
        pos = np.arange(lane, nst, 8)
        out[pos] = pos[::-1]
    return out


def random_valid(nst: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    out = np.arange(padded(nst), dtype=np.uint16)
    for lane in range(8):
        pos = np.arange(lane, nst, 8)
        out[pos] = rng.permutation(pos)
    return out

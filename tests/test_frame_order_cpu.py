"""CPU tests of the frame order's policy as frame_order_ref.py states it (the device builder k_build_frame_order is compared with that
statement in test_frame_order_gpu.py): on random tick arrays the table is a permutation that keeps every position's
% 8 residue, moves neither a position that is not live nor a padded one, and lists a lane's live super-tiles by descending ticks, ties by
position.  The validity predicate, and the switch's argument check (no device needed)."""
import numpy as np
import pytest

import frame_order_ref as ref


def _cases():
    rng = np.random.default_rng(20240611)
    for n in (1, 7, 8, 9, 13, 64, 170, 510, 2040):
        yield n, rng.integers(0, 12000, n).astype(np.uint32)  # 0 .. 120 us, about 4 % below the threshold
        yield n, (rng.integers(0, 3, n) * 450 + rng.integers(0, 2, n) * 100).astype(np.uint32)  # few values around 500: many ties
        yield n, np.where(rng.random(n) < 0.3, rng.integers(500, 9000, n), rng.integers(0, 500, n)).astype(np.uint32)  # a third live


@pytest.mark.parametrize("n,ticks", list(_cases()))
def test_table_properties(n, ticks):
    tab = ref.build_order(ticks)
    npad = ref.padded(n)
    assert tab.dtype == np.uint16 and len(tab) == npad
    assert np.array_equal(np.sort(tab), np.arange(npad)), "a permutation"
    p = np.arange(npad)
    assert np.array_equal(tab & 7, p & 7), "the lane of every position is kept"
    t = np.concatenate([ticks, np.zeros(npad - n, np.uint32)])
    live = t >= ref.LIVE_TICKS
    assert not live[n:].any()
    assert np.array_equal(tab[~live], p[~live]), "positions that are not live, the padded ones among them, keep their super-tile"
    assert live[tab[live]].all(), "live positions get live super-tiles"
    for lane in range(8):
        pos = p[(p & 7) == lane]
        pos = pos[live[pos]]
        e = tab[pos].astype(np.int64)  # the super-tiles at the lane's live positions, in launch order
        te = t[e].astype(np.int64)
        assert (np.diff(te) <= 0).all(), "descending ticks"
        same = np.diff(te) == 0
        assert (np.diff(e)[same] > 0).all(), "ties by position"
    assert ref.is_valid_order(tab, n)


def test_no_live_position_gives_the_identity():
    for n in (1, 8, 13, 510):
        for t in (np.zeros(n, np.uint32), np.full(n, ref.LIVE_TICKS - 1, np.uint32)):
            assert np.array_equal(ref.build_order(t), np.arange(ref.padded(n)))
    # all equal and live: ties by position, the identity again
    assert np.array_equal(ref.build_order(np.full(77, 900, np.uint32)), np.arange(80))
    # one live position has nowhere else to go
    t = np.zeros(510, np.uint32)
    t[255] = 700
    assert np.array_equal(ref.build_order(t), np.arange(512))


def test_a_small_example_by_hand():
    # lane 0 holds positions 0, 8, 16, 24: ticks 600, 100, 900, 600 -> live 0, 16, 24 get 16, 0, 24
    t = np.zeros(30, np.uint32)
    t[[0, 8, 16, 24]] = [600, 100, 900, 600]
    t[[3, 11]] = [500, 499]  # lane 3: one live position stays
    tab = ref.build_order(t)
    exp = np.arange(32)
    exp[[0, 16, 24]] = [16, 0, 24]
    assert np.array_equal(tab, exp)


def test_validity_predicate():
    nst = 13
    ident = np.arange(16, dtype=np.uint16)
    assert ref.is_valid_order(ident, nst)
    assert ref.is_valid_order(ref.reversal(nst), nst) and ref.is_valid_order(ref.random_valid(nst, 5), nst)
    dup = ident.copy()
    dup[8] = 0
    assert not ref.is_valid_order(dup, nst), "a duplicate"
    res = ident.copy()
    res[[0, 1]] = [1, 0]
    assert not ref.is_valid_order(res, nst), "a permutation that changes residues"
    assert not ref.is_valid_order(ident[:8], nst) and not ref.is_valid_order(np.arange(24, dtype=np.uint16), nst), "a wrong length"
    pad = ident.copy()
    pad[[5, 13]] = [13, 5]  # 13 is a padded position of a 13-super-tile shape
    assert not ref.is_valid_order(pad, nst), "a padded position moved"
    assert ref.is_valid_order(pad, 14)
    big = ident.copy()
    big[0] = 16
    assert not ref.is_valid_order(big, nst)
    assert ref.super_tiles(1920, 1080) == 510 and ref.super_tiles(256, 192) == 12 and ref.super_tiles(200, 136) == 12
    assert [ref.super_tiles(256, 192, rank=r, nranks=3) for r in range(3)] == [4, 4, 4]
    assert ref.super_tiles(640, 360, rect=(37, 11, 580, 351)) == 9 * 6


def test_switch_arguments(pkg):
    L = pkg.lib()
    assert L.cgrt_set_frame_order(2) != 0 and L.cgrt_set_frame_order(-2) != 0
    for m in (0, 1, -1):
        pkg.set_frame_order(m)
    for name in ("cgrt_set_frame_order", "cgrt_debug_set_frame_order", "cgrt_debug_get_frame_order", "cgrt_debug_build_frame_order"):
        assert name in pkg.EXPORTS

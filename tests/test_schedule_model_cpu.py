"""tests/helpers/schedule_model.py pinned on cases worked by hand (no GPU, no library).

The model is what tests/test_gpu_schedule.py holds the schedule kernels against, so it is itself checked here against
arrays written out in full.  Tiles are numbered in row order; the costs of the 3x2-tile frame:

    20 x 12 pixels, tiles 0 1 2 over 3 4 5; tile 2 and 5 are 4 pixels wide, tiles 3 4 5 are 4 pixels high
    tile 0: (x 0, y 0) = 1200, (1, 1) = 9, (2, 2) = 3, (4, 4) = 2      tile 1: (8, 0) = 101       tile 2: all 0
    tile 3: (7, 11) = 7          tile 4: (12, 8) = 10          tile 5: (16, 8) = 40, (17, 9) = 8, (18, 10) = 16
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import schedule_model as sm  # noqa: E402

W, H = 20, 12


def _frame():
    c = np.zeros((H, W), np.int64)
    for x, y, v in ((0, 0, 1200), (1, 1, 9), (2, 2, 3), (4, 4, 2), (8, 0, 101), (7, 11, 7), (12, 8, 10), (16, 8, 40),
                    (17, 9, 8), (18, 10, 16)):
        c[y, x] = v
    return c


# (mode, stride) -> keys; stride -> (largest tile work, total work)
KEYS = {
    (0, 1): [1200, 101, 0, 7, 10, 40],
    (0, 2): [1200, 101, 0, 0, 10, 40],
    (0, 4): [1200, 101, 0, 0, 10, 40],
    # m + s // k with k = 64, 64, 32, 32, 32, 16 pixels (stride 1), 16, 16, 8, 8, 8, 4 (2) and 4, 4, 2, 2, 2, 1 (4)
    (1, 1): [1200 + 1214 // 64, 101 + 101 // 64, 0, 7 + 7 // 32, 10 + 10 // 32, 40 + 64 // 16],
    (1, 2): [1200 + 1205 // 16, 101 + 101 // 16, 0, 0, 10 + 10 // 8, 40 + 56 // 4],
    (1, 4): [1200 + 1202 // 4, 101 + 101 // 4, 0, 0, 10 + 10 // 2, 40 + 40 // 1],
    # tile 0's neighbours are 1, 3, 4 (largest 101 -> 75); tiles 1, 3, 4 touch tile 0 (1200 -> 900); tiles 2 and 5 do
    # not (largest neighbour 101 -> 3 * 101 // 4 = 75)
    (2, 1): [1200, 900, 75, 900, 900, 75],
    (2, 2): [1200, 900, 75, 900, 900, 75],
    (2, 4): [1200, 900, 75, 900, 900, 75],
}
KEYS_MODE1_VALUES = {1: [1218, 102, 0, 7, 10, 44], 2: [1275, 107, 0, 0, 11, 54], 4: [1500, 126, 0, 0, 15, 80]}
STATS = {1: (1214, 1214 + 101 + 0 + 7 + 10 + 64), 2: (1205, 1205 + 101 + 0 + 0 + 10 + 56),
         4: (1202, 1202 + 101 + 0 + 0 + 10 + 40)}


def test_mode1_arithmetic_is_what_the_table_says():
    for stride, v in KEYS_MODE1_VALUES.items():
        assert KEYS[(1, stride)] == v


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("stride", (1, 2, 4))
def test_tile_keys_and_stats(mode, stride):
    keys, stats = sm.tile_keys(_frame(), W, H, stride, mode)
    assert keys.tolist() == KEYS[(mode, stride)]
    assert stats == STATS[stride]
    # a pixel the probe did not write is never looked at
    c = _frame()
    probed = np.zeros((H, W), bool)
    probed[::stride, ::stride] = True
    c[~probed] = sm.EMPTY
    keys2, stats2 = sm.tile_keys(c, W, H, stride, mode)
    assert keys2.tolist() == KEYS[(mode, stride)] and stats2 == STATS[stride]


def test_tile_grid_and_single_tiles():
    assert sm.tile_grid(20, 12) == (3, 2) and sm.tile_grid(8, 8) == (1, 1) and sm.tile_grid(9, 1) == (2, 1)
    keys, stats = sm.tile_keys([[7]], 1, 1, 4, 2)          # one pixel, no neighbour
    assert keys.tolist() == [7] and stats == (7, 7)
    keys, stats = sm.tile_keys(np.arange(9).reshape(1, 9), 9, 1, 1, 2)   # tiles of 8 and 1 pixels: 7 | 8
    assert keys.tolist() == [7, 8] and stats == (28, 36)
    keys, _ = sm.tile_keys(np.arange(9).reshape(1, 9) * 2, 9, 1, 1, 2)   # 14 | 16: 3 * 16 // 4 = 12 stays below 14
    assert keys.tolist() == [14, 16]
    keys, _ = sm.tile_keys(np.arange(9).reshape(1, 9) * 3, 9, 1, 1, 2)   # 21 | 24 -> max(21, 18) | 24
    assert keys.tolist() == [21, 24]
    keys, _ = sm.tile_keys([[0] * 8 + [100]], 9, 1, 1, 2)                # 0 | 100 -> 75 | 100
    assert keys.tolist() == [75, 100]


def test_shard_mask_and_counts():
    assert sm.shard_mask([1200, 900, 75, 900, 900, 75], 1, 2).tolist() == [0, 901, 0, 901, 0, 76]
    assert sm.shard_mask([0, 0, 0], 0, 1).tolist() == [1, 1, 1]
    assert sm.shard_mask([5, 6], 6, 7).tolist() == [0, 0]          # fewer tiles than shards: none is this shard's
    assert [sm.shard_tile_count(65, s, 3) for s in range(3)] == [22, 22, 21]
    assert sm.shard_tile_count(2, 6, 7) == 0 and sm.shard_tile_count(2, 1, 7) == 1 and sm.shard_tile_count(1, 0, 1) == 1
    assert sm.shard_tiles(7, 1, 3).tolist() == [1, 4] and sm.shard_tiles(2, 6, 7).tolist() == []


def test_sort_conditions():
    keys = [1100, 1200, 5, 5, 0]
    assert sm.sort_violation([0, 1, 2, 3, 4], keys) is None      # 1100 and 1200 both clamp to 1023: a tie
    assert sm.sort_violation([1, 0, 3, 2, 4], keys) is None
    assert "rises" in sm.sort_violation([2, 0, 1, 3, 4], keys)
    assert "rises" in sm.sort_violation([0, 1, 2, 4, 3], keys)
    assert "permutation" in sm.sort_violation([0, 0, 2, 3, 4], keys)
    assert "permutation" in sm.sort_violation([0, 1, 2, 3, 5], keys)
    assert "entries" in sm.sort_violation([0, 1, 2, 3], keys)
    assert sm.sort_violation([4, 3, 2, 0, 1], keys) is not None   # ascending
    assert sm.a_sorted_order(keys).tolist() == [0, 1, 2, 3, 4]
    assert sm.a_sorted_order([0, 7, 7, 2000, 3]).tolist() == [3, 1, 2, 4, 0]


# The 4x4-tile XCD case: column 1 dominates.  Keys by tile (row order), weights key + 1:
#   column 0: 3 2 1 0 (cost 10)   column 1: 99 199 299 399 (1000)   column 2: 9 9 9 9 (40)   column 3: 4 4 4 4 (20)
XCD_KEYS = [3, 99, 9, 4,
            2, 199, 9, 4,
            1, 299, 9, 4,
            0, 399, 9, 4]


def test_xcd_dominant_column():
    # total 1070; midpoints 5, 510, 1030, 1060 -> * 8 // 1070 = 0, 3, 7, 7
    assert sm.xcd_strips(XCD_KEYS, 4).tolist() == [0, 3, 7, 7]
    order = sm.a_sorted_order(XCD_KEYS)
    assert order.tolist() == [13, 9, 5, 1, 2, 6, 10, 14, 3, 7, 11, 15, 0, 4, 8, 12]
    # strip lists: 0: [0 4 8 12], 3: [13 9 5 1], 7: [2 6 10 14 3 7 11 15]; every group holds 2 slots; the pool is
    # [8 12 | 5 1 | 10 14 3 7 11 15]; groups 1, 2, 4, 5, 6 are empty and take pool entries 0-1, 2-3, 4-5, 6-7, 8-9
    got = sm.xcd_order(order, XCD_KEYS, 4)
    assert got.tolist() == [0, 8, 5, 13, 10, 3, 11, 2,
                            4, 12, 1, 9, 14, 7, 15, 6]
    assert sm.slot_pairs(got, XCD_KEYS, 4).tolist() == [
        [0, 3], [0, 1], [3, 199], [3, 399], [7, 9], [7, 4], [7, 4], [7, 9],
        [0, 2], [0, 0], [3, 99], [3, 299], [7, 9], [7, 4], [7, 4], [7, 9]]


def test_xcd_clamps_the_weights():
    # keys above 1023 weigh 1024: two columns of one tile each, 5000 | 1023 -> equal costs, strips 2 and 6
    assert sm.xcd_strips([5000, 1023], 2).tolist() == [2, 6]
    assert sm.xcd_strips([1], 1).tolist() == [4]            # one column of weight 2: midpoint 1 of 2, the middle strip
    assert sm.xcd_strips([0], 1).tolist() == [0]            # weight 1: the midpoint 1 // 2 = 0


def test_xcd_guards():
    assert sm.xcd_applies(64, 64) and sm.xcd_applies(100, 37) and sm.xcd_applies(8, 64) and sm.xcd_applies(16384, 8)
    assert not sm.xcd_applies(16392, 8)        # 2049 tile columns
    assert not sm.xcd_applies(1, 17)           # 17 pixels, 3 tiles: fewer than 9 pixels per tile
    assert not sm.xcd_applies(9, 1)
    assert not sm.xcd_applies(64, 64, shards=2)


@pytest.mark.parametrize("n_tiles,tiles_x", ((1, 1), (9, 3), (64, 8), (65, 13), (72, 9), (80, 10), (1089, 33)))
def test_xcd_pairs_do_not_depend_on_the_tie_break(n_tiles, tiles_x):
    rng = np.random.default_rng(7)
    col = np.arange(n_tiles) % tiles_x
    layouts = (rng.integers(0, 5, n_tiles), rng.integers(0, 3001, n_tiles), np.zeros(n_tiles, np.int64),
               np.where(col == tiles_x // 2, 500, 0) + rng.integers(0, 2, n_tiles))
    for keys in layouts:
        want = sm.xcd_order(sm.a_sorted_order(keys), keys, tiles_x)
        assert np.array_equal(np.sort(want), np.arange(n_tiles))
        pairs = sm.slot_pairs(want, keys, tiles_x)
        for _ in range(6):
            order = sm.a_sorted_order(keys, rng)
            assert sm.sort_violation(order, keys) is None
            got = sm.xcd_order(order, keys, tiles_x)
            assert np.array_equal(np.sort(got), np.arange(n_tiles))
            assert np.array_equal(sm.slot_pairs(got, keys, tiles_x), pairs)


def test_expansion():
    E = sm.EMPTY
    # 9x1: tile 1 is the single pixel 8, tile 0 the pixels 0..7 in its first row
    got = sm.expand_slots([1, 0], 9, 1)
    assert got.tolist() == [8] + [E] * 63 + list(range(8)) + [E] * 56
    # 10x9, tiles 0 1 over 2 3: tile 3 starts at (8, 8) and holds pixels 88, 89
    got = sm.expand_slots([3], 10, 9)
    assert got.tolist() == [88, 89] + [E] * 62
    got = sm.expand_slots([1], 10, 9)          # x 8..9, y 0..7
    assert got.tolist() == sum(([10 * y + 8, 10 * y + 9] + [E] * 6 for y in range(8)), [])

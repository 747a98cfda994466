"""The residual-block kernel's tile table (csrc/resblock.hip: rb_build_rows), through the host-only entry y4_rb_tile_table: the cut of
every column into allowed heights and the deal of the tiles to the workgroups' lists, checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

from yolo4hip import ext

HEIGHTS = {128: (16, 12, 8, 4), 64: (16, 8)}
# a tile's cost a + b * rows in cycles, from the phase trace of the full tiles (LABNOTES.md section 4.1c: 45.9 k cycles at C = 128, 22.2 k
# at C = 64; the 3x3 loop, the epilogue and 16 of the 1x1 phase's 18 rows scale with rows): pinned here, not taken from the table
COST = {128: (6700, 2450), 64: (3240, 1185)}
SQUARES = (12, 20, 24, 28, 36, 40, 52, 76, 104, 152)
SHAPES = [(s, s) for s in SQUARES] + [(36, 52), (24, 76)]


def table(n, h, w, c, slots):
    """-> (grid, stride, a, b, lists): lists[i] = the (image, first row, rows, tile column) entries of workgroup i"""
    lib = ext.load()
    count = lib.y4_rb_tile_table(n, h, w, c, slots, None, 0)
    assert count > 4 and count % 4 == 0, count
    buf = (C.c_int32 * count)()
    assert lib.y4_rb_tile_table(n, h, w, c, slots, buf, count) == count
    v = np.frombuffer(buf, dtype=np.int32).reshape(-1, 4)
    grid, stride, a, b = (int(x) for x in v[0])
    assert v.shape[0] == 1 + grid * stride
    lists = []
    for i in range(grid):
        rows = v[1 + i * stride: 1 + (i + 1) * stride]
        ends = np.nonzero(rows[:, 2] == 0)[0]
        assert len(ends) > 0, "every list is closed by an entry with rows = 0"
        assert not rows[ends[0]:].any(), "nothing behind a list's end"
        lists.append([tuple(int(x) for x in e) for e in rows[:ends[0]]])
    return grid, stride, a, b, lists


def check_table(n, h, w, c, slots):
    grid, stride, a, b, lists = table(n, h, w, c, slots)
    hs, hmin = HEIGHTS[c], min(HEIGHTS[c])
    assert 8 <= grid <= slots and grid % 8 == 0
    assert (a, b) == COST[c]
    tiles_x = (w + 15) // 16
    cover = np.zeros((n, tiles_x, h + 16), dtype=np.int32)          # per image and tile column: how often each row is computed
    for lst in lists:
        for img, y0, rows, tx in lst:
            assert rows in hs, (rows, hs)
            assert 0 <= img < n and 0 <= tx < tiles_x and 0 <= y0 < h, "no tile starts outside the map"
            cover[img, tx, y0:y0 + rows] += 1
    # every output row of every column of every image exactly once (so every tile is in exactly one list) ...
    assert (cover[:, :, :h] == 1).all()
    # ... and what hangs over the lower edge is less than the smallest height, once, and nothing where h is a multiple of it
    dead = cover[:, :, h:].sum(axis=2)
    assert (cover[:, :, h:] <= 1).all() and (dead <= hmin - 1).all()
    assert (dead == (-h) % hmin).all()
    # the deal: the longest list costs at most the mean over the slots plus one full tile
    full = a + 16 * b
    cost = [sum(a + b * rows for _, _, rows, _ in lst) for lst in lists]
    total = sum(cost)
    assert max(cost) <= total / slots + full, (max(cost) / full, total / slots / full)
    # list i runs on XCD i % 8, and the XCDs take contiguous ranges of the tiles in (image, row, column) order
    last = None
    for x in range(8):
        mine = sorted((img, y0, tx) for i in range(x, grid, 8) for img, y0, _, tx in lists[i])
        if mine:
            assert last is None or last < mine[0]
            last = mine[-1]
    return max(cost) / full, total / slots / full


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("h,w", SHAPES)
def test_tile_table_covers_and_balances(h, w, c):
    for n in (1, 2, 5, 32):
        for slots in (8, 256, 512):
            check_table(n, h, w, c, slots)


def test_headline_shape_is_one_balanced_round():
    """76 x 76, batch 32, C = 128 on 256 workgroups: 640 full and 160 twelve-row tiles are 12 160 output rows, 47.5 per list; lists such
    as [16 16 16] and [12 12 12 12] hold them in one round, and no list is costlier than 3.25 full tiles."""
    longest, mean = check_table(32, 76, 76, 128, 256)
    print(f"longest list {longest:.3f} full tiles, mean {mean:.3f}")
    assert longest <= 3.25
    grid, stride, a, b, lists = table(32, 76, 76, 128, 256)
    assert max(sum(rows for _, _, rows, _ in lst) for lst in lists) <= 48, "no list longer than three full tiles' rows"
    assert grid == 256 and sum(rows for lst in lists for _, _, rows, _ in lst) == 32 * 5 * 76


def test_fewer_tiles_than_slots_are_cut_further():
    """One 76 x 76 image is 25 full-height tiles for 256 workgroups: the table cuts them into short tiles instead (as the earlier
    part tiles did), so that more compute units share the image."""
    grid, stride, a, b, lists = table(1, 76, 76, 128, 256)
    assert sum(1 for lst in lists if lst) > 25 and max(len(lst) for lst in lists) == 1


def test_bad_arguments_are_errors():
    lib = ext.load()
    for args in ((0, 76, 76, 128, 256), (1, 76, 76, 96, 256), (1, 76, 76, 128, 4), (1, 76, 76, 128, 12), (1, 0, 76, 64, 8)):
        assert lib.y4_rb_tile_table(*args, None, 0) < 0

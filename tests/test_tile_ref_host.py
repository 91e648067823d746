"""tests/tile_ref.py on cases worked out by hand (no GPU): the reference the tile-scheduler tests trust is checked here first."""
import numpy as np
import pytest

from mort_amd import hip
from tests import tile_ref as T


def test_tile_costs_by_hand():
    # 10 x 9 packed rows: tiles_x = 2, tiles_y = 2.  Tile 0 = rows 0-7 x cols 0-7, tile 1 = rows 0-7 x cols 8-9,
    # tile 2 = row 8 x cols 0-7, tile 3 = row 8 x cols 8-9.
    seg = np.ones((9, 10), dtype=np.uint32)
    seg[0, 0] = 7       # tile 0
    seg[7, 7] = 5       # tile 0 (its last pixel)
    seg[7, 8] = 11      # tile 1 (first column of the ragged tile)
    seg[8, 7] = 13      # tile 2
    seg[8, 9] = 17      # tile 3 (the corner tile: 1 row x 2 columns)
    assert T.tile_costs(seg, 10, "max").tolist() == [7, 11, 13, 17]
    # sums: tile 0 = 64 ones + 6 + 4 = 74; tile 1 = 16 ones + 10 = 26; tile 2 = 8 ones + 12 = 20; tile 3 = 2 ones + 16 = 18
    assert T.tile_costs(seg, 10, "sum").tolist() == [74, 26, 20, 18]
    assert T.tile_costs(seg.reshape(-1), 10, "max").tolist() == [7, 11, 13, 17]  # flat input, the same rows
    assert T.tile_costs(seg, 10).dtype == np.uint32
    # a sum past 2^32 wraps as the device's 32-bit atomicAdd does: 2 x 0x80000001 = 2^32 + 2 -> 2
    big = np.zeros((1, 2), dtype=np.uint32) + np.uint32(0x80000001)
    assert T.tile_costs(big, 2, "sum").tolist() == [2] and T.tile_costs(big, 2, "max").tolist() == [0x80000001]
    with pytest.raises(ValueError):
        T.tile_costs(seg, 10, "mean")


def test_tile_costs_are_of_packed_local_rows():
    # rank 1 of 2 with 8-row blocks of a 24-row image owns image rows 8-15 only: ONE tile row, whatever the image rows are called
    seg = np.arange(8 * 8, dtype=np.uint32).reshape(8, 8)
    assert T.tile_costs(seg, 8, "max").tolist() == [63]


def test_order_desc_by_hand():
    # costs 5 9 5 0 9: the two 9s first (index 1 before 4), then the two 5s (0 before 2), then the 0
    keys, order = T.order_desc([5, 9, 5, 0, 9])
    assert order.tolist() == [1, 4, 0, 2, 3] and keys.tolist() == [9, 9, 5, 5, 0]
    assert order.dtype == np.uint32 and keys.dtype == np.uint32
    # all equal: the identity
    assert T.order_desc([3] * 6)[1].tolist() == [0, 1, 2, 3, 4, 5]
    # unsigned: a value with bit 31 set sorts above 0x7fffffff
    keys, order = T.order_desc([0x7fffffff, 0xffffffff, 0x80000000, 1])
    assert order.tolist() == [1, 2, 0, 3] and keys.tolist() == [0xffffffff, 0x80000000, 0x7fffffff, 1]
    assert T.order_desc([42])[1].tolist() == [0]


def test_heavy_head_by_hand():
    keys = [100, 60, 50, 49, 10, 0, 0]
    # chain-bound: top * lanes = 100 * 64 = 6400 >= 2 * 3200.  50 %: threshold ceil(50) = 50 -> 100, 60, 50 reach it
    assert T.heavy_head(keys, 50, 99, 3200, 64) == 3
    assert T.heavy_head(keys, 50, 2, 3200, 64) == 2          # clamped to max_r
    # one segment more in the total: 6400 < 6402 -> not chain-bound
    assert T.heavy_head(keys, 50, 99, 3201, 64) == 0
    assert T.heavy_head(keys, 50, 99, 3199, 64) == 3
    assert T.heavy_head(keys, 50, 99, 0, 64) == 0            # no total: no head
    # the threshold rounds UP: 49 % of 100 = 49 -> 49 reaches it; 49 % of 101 = 49.49 -> 50, and 49 does not
    assert T.heavy_head(keys, 49, 99, 1, 64) == 4
    assert T.heavy_head([101, 60, 50, 49], 49, 99, 1, 64) == 3
    # 1 %: threshold ceil(1.0) = 1 -> every non-zero key; the zeros never count, not even at a threshold of 0
    assert T.heavy_head(keys, 1, 99, 1, 64) == 5
    assert T.heavy_head(keys, 0, 99, 1, 64) == 5
    assert T.heavy_head(keys, 100, 99, 1, 64) == 1
    # all keys zero: top * lanes = 0 < 2 * total for any total > 0
    assert T.heavy_head([0, 0, 0], 50, 99, 1, 1 << 40) == 0
    # no 32- or 64-bit wrap: top = 2^32 - 1, lanes = 2^33 -> top * lanes ~ 2^65
    assert T.heavy_head([0xffffffff, 1], 50, 99, 1 << 63, 1 << 33) == 1
    assert T.heavy_head([0xffffffff, 1], 50, 99, (1 << 64) - 1, 1 << 33) == 0   # 2 * total ~ 2^65 > (2^32 - 1) * 2^33


def test_counters_total_by_hand():
    c = np.zeros(96, dtype=np.uint64)
    c[0] = 5
    c[32] = 7       # slot of workgroup 0
    c[94] = 11      # slot of workgroup 31
    c[33] = 1000    # a draw count: ignored
    c[1] = c[2] = c[3] = 999  # draws, work cursor, walks: ignored
    assert T.counters_total(c) == 23


def test_deinterleave_by_hand():
    # W = 1, H = 5, two ranks, 2-row blocks: blocks {0,1}, {2,3}, {4}; rank 0 owns blocks 0 and 2 = image rows 0 1 4 (packed 0 1 2),
    # rank 1 owns block 1 = rows 2 3.  The gather stride is ceil(3 blocks / 2 ranks) * 2 rows = 4 pixels.
    stride = 4
    P = 0xdeadbeef  # padding
    g = np.array([10, 11, 14, P, 12, 13, P, P], dtype=np.uint32)
    assert T.deinterleave(g, 1, 5, 2, 2, stride).reshape(-1).tolist() == [10, 11, 12, 13, 14]
    # one rank: the identity
    assert T.deinterleave(np.arange(6, dtype=np.uint32), 2, 3, 1, 8, 6).tolist() == [[0, 1], [2, 3], [4, 5]]
    # more ranks than blocks: rank 1 of 2 owns nothing of a 2-row image with 8-row blocks
    g = np.array([1, 2] + [P] * 6 + [P] * 8, dtype=np.uint32)
    assert T.deinterleave(g, 1, 2, 2, 8, 8).reshape(-1).tolist() == [1, 2]


def test_gather_stride_is_the_library_s_and_holds_every_rank():
    """The library's stride (comm_rccl.hip gather_tile_px, host arithmetic: no GPU needed) is the largest packed tile, blocks counted whole."""
    from mort_amd import partition
    for (W, H, N, rpb) in [(7, 5, 1, 8), (64, 64, 2, 8), (97, 55, 3, 8), (33, 100, 8, 8), (16, 9, 4, 16), (300, 77, 2, 16)]:
        stride = hip.debug_gather_stride(W, H, N, rpb)
        assert stride == partition.max_local_rows(H, N, rpb) * W
        assert all(partition.local_rows(H, r, N, rpb) * W <= stride for r in range(N))
    # (97, 55, 3, 8) by hand: 7 blocks, ceil(7 / 3) = 3 blocks of 8 rows = 24 rows of 97 pixels
    assert hip.debug_gather_stride(97, 55, 3, 8) == 24 * 97

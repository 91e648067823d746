"""Plain restatements of what the tile scheduler computes on the device (numpy and Python ints only; tests/test_tile_ref_host.py
checks them on hand-worked cases, tests/test_gpu_tile_state.py compares the device with them, always by exact equality):

 - tile_costs:   pixel_write's per-tile keys (mega_bvh.h) -- the longest pixel, or the sum, of every 8x8 tile of the PACKED LOCAL rows;
 - order_desc:   tile_sort.hip's argsort -- descending, equal costs in index order;
 - heavy_head:   heavy_count_kernel's rule (DESIGN.md 5 "Heavy waves");
 - deinterleave: comm_rccl.hip's gather layout -> frame, from mort_amd.partition's row arithmetic."""
import numpy as np

from mort_amd import partition

TILE = 8
COUNTERS = 96


def tile_costs(seg_rows, W, key="max"):
    """seg_rows: the per-pixel segment counts of a partition's packed local rows, (local_rows, W) or flat.  Returns the cost of every
    8x8 tile, row-major over ceil(local_rows / 8) x ceil(W / 8) tiles, as uint32 (the sum wraps at 2^32 as atomicAdd does)."""
    seg = np.asarray(seg_rows, dtype=np.uint64).reshape(-1, W)
    rows = seg.shape[0]
    tx, ty = (W + TILE - 1) // TILE, (rows + TILE - 1) // TILE
    padded = np.zeros((ty * TILE, tx * TILE), dtype=np.uint64)
    padded[:rows, :W] = seg
    blocks = padded.reshape(ty, TILE, tx, TILE)
    if key == "max":
        cost = blocks.max(axis=(1, 3))
    elif key == "sum":
        cost = blocks.sum(axis=(1, 3)) & np.uint64(0xffffffff)
    else:
        raise ValueError(key)
    return cost.reshape(-1).astype(np.uint32)


def order_desc(cost):
    """Stable descending argsort: order[i] = index of the i-th largest cost, equal costs by increasing index.  (keys, order)."""
    cost = np.asarray(cost, dtype=np.uint32).reshape(-1)
    order = sorted(range(cost.size), key=lambda i: (-int(cost[i]), i))
    order = np.array(order, dtype=np.uint32)
    return cost[order], order


def counters_total(counters):
    """the segment total heavy_count_kernel takes from 96 saved counters: word 0 plus the 32 per-workgroup slots 32 + 2 k (the odd
    words beside them are draw counts)"""
    c = [int(v) for v in np.asarray(counters).reshape(-1)]
    assert len(c) == COUNTERS
    return c[0] + sum(c[32 + 2 * k] for k in range(32))


def heavy_head(keys, percent, max_r, total, lanes):
    """How many tiles of the descending `keys` form the heavy-wave head: those that reach ceil(top * percent / 100) and are not zero, at
    most max_r -- or none unless the frame the keys come from was chain-bound: total > 0 and top * lanes >= 2 * total (its longest
    pixel at least twice an average lane's share).  Unbounded ints throughout."""
    keys = [int(k) for k in np.asarray(keys).reshape(-1)]
    top = keys[0]
    total, lanes = int(total), int(lanes)
    if not (total > 0 and top * lanes >= 2 * total):
        return 0
    thr = -((-top * int(percent)) // 100)
    count = sum(1 for k in keys if k >= thr and k > 0)
    return min(count, int(max_r))


def deinterleave(gathered, W, H, nranks, rpb, stride):
    """gathered: (nranks * stride,) uint32 pixels, rank r's packed rows from r * stride on.  Returns the (H, W) uint32 frame: packed row
    l of rank r is image row partition.global_rows(r, ...)[l]; rows past the image (padding) are not read."""
    g = np.asarray(gathered, dtype=np.uint32).reshape(-1)
    assert g.size == nranks * stride
    frame = np.zeros((H, W), dtype=np.uint32)
    seen = np.zeros(H, dtype=np.int64)
    for r in range(nranks):
        n = partition.local_rows(H, r, nranks, rpb)
        rows = np.asarray(partition.global_rows(r, nranks, rpb, n)).astype(np.int64).reshape(-1)
        assert n * W <= stride and (rows < H).all()
        tile = g[r * stride: r * stride + n * W].reshape(n, W)
        frame[rows] = tile
        seen[rows] += 1
    assert (seen == 1).all()
    return frame

"""The contract of the irradiance volumes (include/mort_hip.h) restated in numpy float32, and nothing else: the
probe positions, the record layout, and one sample -- cell and fractions per axis, the basis products, the eight corners in
ascending order, the 9-term sum from the k = 0 product, the accumulation from 0.0f and the division by the weights' sum.  Every
operation is one float32 numpy operation on float32 operands, so every intermediate is rounded where the contract rounds it."""
import numpy as np

F = np.float32
RECORD_FLOATS = 32
C0, C1, C2, C3, C4 = F(0.2820948), F(0.4886025), F(1.0925484), F(0.31539157), F(0.5462742)
A = (F(np.pi), F(2.0 * np.pi / 3.0), F(np.pi / 4.0))
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)


def grid_arrays(grid):
    """(origin, spacing, count) of a grid given as a hip.VOLUME_GRID or as a tuple (origin, spacing, count[, time])"""
    if isinstance(grid, tuple):
        return np.asarray(grid[0], dtype=F), np.asarray(grid[1], dtype=F), [int(c) for c in grid[2]]
    return np.array(list(grid.origin), dtype=F), np.array(list(grid.spacing), dtype=F), [int(c) for c in grid.count]


def positions(grid):
    """float32 (probes, 3) in index order p = (iz ny + iy) nx + ix: origin[a] + (float)i_a * spacing[a], product rounded, then sum"""
    origin, spacing, count = grid_arrays(grid)
    iz, iy, ix = np.meshgrid(np.arange(count[2]), np.arange(count[1]), np.arange(count[0]), indexing="ij")
    idx = np.stack([ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)], axis=1).astype(F)
    step = (idx * spacing[None, :]).astype(F)
    return (origin[None, :] + step).astype(F)


def pack(sh, weight=None):
    """float32 (n, 32): the 27 words as they are, the weight (None = 1.0f), four 0.0f"""
    sh = np.ascontiguousarray(sh, dtype=F).reshape(-1, 27)
    rec = np.zeros((sh.shape[0], RECORD_FLOATS), dtype=F)
    rec.view(np.uint32)[:, :27] = sh.view(np.uint32)
    rec[:, 27] = F(1.0) if weight is None else np.asarray(weight, dtype=F).reshape(-1)
    return rec


def basis(normal):
    """B_k = A_l(k) * Y_k(n), float32 (n, 9); the normal as given"""
    n = np.asarray(normal, dtype=F).reshape(-1, 3)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    Y = [np.full(len(n), C0, dtype=F), C1 * y, C1 * z, C1 * x, (C2 * x) * y, (C2 * y) * z, C3 * ((F(3.0) * z) * z - F(1.0)), (C2 * x) * z,
         C4 * (x * x - y * y)]
    return np.stack([(A[BAND[k]] * Y[k]).astype(F) for k in range(9)], axis=1)


def axis(x, origin, inv, count):
    """(i0, i1, w0, w1) along one axis for float32 coordinates x"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((x - origin).astype(F) * inv).astype(F)
        u = np.where(u > 0, u, F(0.0)).astype(F)  # NaN goes to 0
        m = F(count - 1)
        u = np.where(u < m, u, m).astype(F)
    i0 = np.floor(u).astype(np.int64)
    i0 = np.where(i0 > count - 2, count - 2, i0)
    i0 = np.where(i0 < 0, 0, i0)
    f = (u - i0.astype(F)).astype(F)
    i1 = np.where(i0 + 1 < count, i0 + 1, i0)
    return i0, i1, (F(1.0) - f).astype(F), f


def sample(grid, records, points, normals, census=None):
    """float32 (n, 4) = {acc * r, wsum} per point.  census: a list that receives the number of contributing corners per point."""
    origin, spacing, count = grid_arrays(grid)
    rec = np.ascontiguousarray(records, dtype=F).reshape(-1, RECORD_FLOATS)
    assert rec.shape[0] == count[0] * count[1] * count[2]
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    n = len(p)
    inv = (F(1.0) / spacing).astype(F)
    ax = [axis(p[:, a], origin[a], inv[a], count[a]) for a in range(3)]
    B = basis(normals)
    acc = np.zeros((n, 3), dtype=F)
    wsum = np.zeros(n, dtype=F)
    used = np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for c in range(8):
            cx, cy, cz = c & 1, (c >> 1) & 1, c >> 2
            T = ((ax[0][2 + cx] * ax[1][2 + cy]).astype(F) * ax[2][2 + cz]).astype(F)
            idx = (ax[2][cz] * count[1] + ax[1][cy]) * count[0] + ax[0][cx]
            r = rec[idx]
            W = (T * r[:, 27]).astype(F)
            on = W > 0
            e = (B[:, 0, None] * r[:, 0:3]).astype(F)
            for k in range(1, 9):
                e = (e + (B[:, k, None] * r[:, 3 * k:3 * k + 3]).astype(F)).astype(F)
            acc = np.where(on[:, None], (acc + (W[:, None] * e).astype(F)).astype(F), acc)
            wsum = np.where(on, (wsum + W).astype(F), wsum)
            used += on
        ok = wsum > 0
        r = (F(1.0) / np.where(ok, wsum, F(1.0))).astype(F)
        out = np.zeros((n, 4), dtype=F)
        out[:, :3] = np.where(ok[:, None], (acc * r[:, None]).astype(F), F(0.0))
        out[:, 3] = np.where(ok, wsum, F(0.0))
    if census is not None:
        census.append(used)
    return out

"""The contract of the visibility-weighted irradiance volumes (include/mort_hip.h) restated in numpy float32, and
nothing else: the octahedral directions of a depth map's sub-samples, the two moments per texel, the border copies, and one
sample with every corner's weight multiplied by the Chebyshev visibility.  Every operation is one float32 numpy operation on
float32 operands, so every intermediate is rounded where the contract rounds it.  The distances come from the oracle
(tests/query_rays.oracle_closest), never from the library."""
import numpy as np

from tests import query_rays as Q
from tests.volume_ref import RECORD_FLOATS, axis, basis, grid_arrays, positions  # noqa: F401  (positions: for the callers)

F = np.float32
R = 8
SIDE = R + 2
DEPTH_FLOATS = 2 * SIDE * SIDE
ONE, HALF = F(1.0), F(0.5)


def octahedral(u, v):
    """(x, y, z) float32 of float32 (u, v) in [-1, 1]^2, not normalised"""
    au, av = np.abs(u), np.abs(v)
    z = ((ONE - au) - av).astype(F)
    fold = z < 0
    x = np.where(fold, (ONE - av) * np.where(u >= 0, ONE, -ONE), u).astype(F)
    y = np.where(fold, (ONE - au) * np.where(v >= 0, ONE, -ONE), v).astype(F)
    return x, y, z


def directions(s):
    """float32 (64, s * s, 3): texel lane = j * 8 + i, within a texel the sub-samples in ascending b and within b ascending a"""
    step = F(2.0) / F(R * s)
    lane = np.arange(R * R)
    i, j = lane % R, lane // R
    sub = np.arange(s * s)
    a, b = sub % s, sub // s
    u = ((i[:, None] * s + a[None, :]).astype(F) + HALF) * step - ONE
    v = ((j[:, None] * s + b[None, :]).astype(F) + HALF) * step - ONE
    assert u.dtype == F and v.dtype == F
    return np.stack(octahedral(u, v), axis=2)


def borders(interior):
    """float32 (n, 10, 10, 2) indexed [p, j, i] from the interior (n, 8, 8, 2): the border texels are copies"""
    n = interior.shape[0]
    m = np.zeros((n, SIDE, SIDE, 2), dtype=F)
    m[:, 1:R + 1, 1:R + 1] = interior
    for k in range(1, R + 1):
        m[:, k, 0] = m[:, R + 1 - k, 1]          # (0, j) <- (1, 9 - j)
        m[:, k, R + 1] = m[:, R + 1 - k, R]      # (9, j) <- (8, 9 - j)
        m[:, 0, k] = m[:, 1, R + 1 - k]          # (i, 0) <- (9 - i, 1)
        m[:, R + 1, k] = m[:, R, R + 1 - k]      # (i, 9) <- (9 - i, 8)
    m[:, 0, 0] = m[:, R, R]
    m[:, R + 1, R + 1] = m[:, 1, 1]
    m[:, R + 1, 0] = m[:, 1, R]                  # (0, 9) <- (8, 1)
    m[:, 0, R + 1] = m[:, R, 1]                  # (9, 0) <- (1, 8)
    return m


def moments(dirs, t, hit, max_distance):
    """float32 (n, 8, 8, 2) from the oracle's t and hit flags, both (n, 64, s * s), and the directions (64, s * s, 3)"""
    mx = F(max_distance)
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    length = np.sqrt((x * x + y * y) + z * z)
    assert length.dtype == F
    n, s2 = t.shape[0], t.shape[2]
    m1 = np.zeros((n, R * R), dtype=F)
    m2 = np.zeros((n, R * R), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(s2):
            d = np.where(hit[:, :, k], t[:, :, k] * length[None, :, k], mx).astype(F)
            d = np.where(d < mx, d, mx).astype(F)  # a NaN goes to the cap
            m1 = m1 + d
            m2 = m2 + d * d
    inv = ONE / F(s2)
    out = np.stack([m1 * inv, m2 * inv], axis=2)
    assert out.dtype == F
    return out.reshape(n, R, R, 2)


def bake(world, probes, s, max_distance):
    """float32 (n, 200): the maps of PROBE_DTYPE probes over the oracle's closest hits, media passed over"""
    n = len(probes)
    dirs = directions(s)
    rays = np.zeros((n, R * R, s * s, 8), dtype=F)
    rays[..., 0:3] = probes["position"][:, None, None, :]
    rays[..., 3:6] = dirs[None]
    rays[..., 6] = probes["time"][:, None, None]
    rays[..., 7] = np.inf
    rec, hit = Q.oracle_closest(world, rays.reshape(-1, 8))
    shape = (n, R * R, s * s)
    return borders(moments(dirs, rec["t"].astype(F).reshape(shape), hit.reshape(shape), max_distance)).reshape(n, DEPTH_FLOATS)


def _coord(o):
    t = (o * HALF + HALF) * F(R) + HALF
    i0 = np.clip(np.floor(t).astype(np.int64), 0, R)
    return i0, (t - i0.astype(F)).astype(F)


def visibility(maps, p, v, min_visibility, census=None):
    """V float32 (n,) of probe indices p (n,) for the offsets v (n, 3) = q - pos; maps (probes, 10, 10, 2) indexed [p, j, i]"""
    v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
    r = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
    s1 = (np.abs(v0) + np.abs(v1)) + np.abs(v2)
    ok = (s1 > 0) & (s1 < np.inf)
    safe = np.where(ok, s1, ONE)
    ox = np.where(ok, v0 / safe, F(0.0)).astype(F)
    oy = np.where(ok, v1 / safe, F(0.0)).astype(F)
    fold = ok & (v2 < 0)
    fx_ = (ONE - np.abs(oy)) * np.where(ox >= 0, ONE, -ONE)
    fy_ = (ONE - np.abs(ox)) * np.where(oy >= 0, ONE, -ONE)
    ox, oy = np.where(fold, fx_, ox).astype(F), np.where(fold, fy_, oy).astype(F)
    i0, fx = _coord(ox)
    j0, fy = _coord(oy)
    gx, gy = ONE - fx, ONE - fy
    m = []
    for k in range(2):
        t = maps[..., k]
        top = t[p, j0, i0] * gx + t[p, j0, i0 + 1] * fx
        bot = t[p, j0 + 1, i0] * gx + t[p, j0 + 1, i0 + 1] * fx
        m.append(top * gy + bot * fy)
    m1, m2 = m
    var = np.abs(m2 - m1 * m1)
    dl = r - m1
    den = var + dl * dl
    k = np.where(den > 0, var / np.where(den > 0, den, ONE), F(0.0)).astype(F)
    V = (k * k) * k
    V = np.where(V > F(min_visibility), V, F(min_visibility)).astype(F)
    beyond = ok & (r > m1)
    V = np.where(beyond, V, ONE).astype(F)
    assert V.dtype == F and r.dtype == F and m1.dtype == F
    if census is not None:
        census.append((beyond, V < 1))
    return V


def sample_visible(grid, records, depth, normal_bias, min_visibility, points, normals, census=None, shares=None):
    """float32 (n, 4) = {acc * r, wsum} per point.  census: a dict that receives the counts of corner evaluations (W0 > 0), of
    those with r > m1 and of those that end with V < 1.  shares: a list that receives W_c per corner, (8, n), 0 where skipped."""
    origin, spacing, count = grid_arrays(grid)
    rec = np.ascontiguousarray(records, dtype=F).reshape(-1, RECORD_FLOATS)
    probes = count[0] * count[1] * count[2]
    assert rec.shape[0] == probes
    maps = np.ascontiguousarray(depth, dtype=F).reshape(probes, SIDE, SIDE, 2)
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=F).reshape(-1, 3)
    n = len(p)
    inv = (ONE / spacing).astype(F)
    ax = [axis(p[:, a], origin[a], inv[a], count[a]) for a in range(3)]
    B = basis(nrm)
    acc = np.zeros((n, 3), dtype=F)
    wsum = np.zeros(n, dtype=F)
    evaluated = beyond_n = dimmed_n = 0
    per_corner = np.zeros((8, n), dtype=F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        q = (p + (F(normal_bias) * nrm).astype(F)).astype(F)
        for c in range(8):
            cs = (c & 1, (c >> 1) & 1, c >> 2)
            T = ((ax[0][2 + cs[0]] * ax[1][2 + cs[1]]).astype(F) * ax[2][2 + cs[2]]).astype(F)
            ii = [ax[a][cs[a]] for a in range(3)]
            idx = (ii[2] * count[1] + ii[1]) * count[0] + ii[0]
            r = rec[idx]
            W0 = (T * r[:, 27]).astype(F)
            on0 = W0 > 0
            pos = np.stack([(origin[a] + (ii[a].astype(F) * spacing[a]).astype(F)).astype(F) for a in range(3)], axis=1)
            seen = []
            V = visibility(maps, idx, (q - pos).astype(F), min_visibility, census=seen)
            W = (W0 * V).astype(F)
            on = on0 & (W > 0)
            evaluated += int(on0.sum()); beyond_n += int((on0 & seen[0][0]).sum()); dimmed_n += int((on0 & seen[0][1]).sum())
            e = (B[:, 0, None] * r[:, 0:3]).astype(F)
            for k in range(1, 9):
                e = (e + (B[:, k, None] * r[:, 3 * k:3 * k + 3]).astype(F)).astype(F)
            acc = np.where(on[:, None], (acc + (W[:, None] * e).astype(F)).astype(F), acc)
            wsum = np.where(on, (wsum + W).astype(F), wsum)
            per_corner[c] = np.where(on, W, F(0.0))
        ok = wsum > 0
        rr = (ONE / np.where(ok, wsum, ONE)).astype(F)
        out = np.zeros((n, 4), dtype=F)
        out[:, :3] = np.where(ok[:, None], (acc * rr[:, None]).astype(F), F(0.0))
        out[:, 3] = np.where(ok, wsum, F(0.0))
    if census is not None:
        census.update(evaluated=evaluated, beyond=beyond_n, dimmed=dimmed_n)
    if shares is not None:
        shares.append(per_corner)
    return out

"""Inputs the irradiance-volume tests share (tests/test_volume_host.py, tests/test_gpu_volume.py): the grids, records under the
three kinds of mask, the points and normals of the parity tests, the scene-6 hits.  Nothing here computes an expected answer:
that is tests/volume_ref.py."""
import functools

import numpy as np

from mort_amd import hip, host
from tests import query_rays as Q
from tests import volume_ref as V
from tests.feature_ref import primary_rays

F = np.float32
COUNTS = [(1, 1, 1), (2, 1, 3), (4, 3, 2), (5, 4, 3)]
ORIGIN, SPACING = (-1.5, 0.25, 3.0), (0.7, 1.3, 0.45)


def grid(count, origin=ORIGIN, spacing=SPACING, time=0.5):
    return hip.VOLUME_GRID(origin, spacing, count, time)


def box(g):
    """(lo, hi) float64 of the probes' box"""
    origin, spacing, count = V.grid_arrays(g)
    lo = origin.astype(np.float64)
    return lo, lo + spacing.astype(np.float64) * (np.array(count) - 1)


def coefficients(g, seed=1):
    """float32 (probes, 27) in [-1, 2)"""
    return np.random.default_rng(seed).uniform(-1.0, 2.0, size=(g.probes, 27)).astype(F)


def records(g, mask="ones", seed=1):
    """float32 (probes, 32) by the restated layout.  mask: "ones"; "fractional" = weights in (0, 2), a quarter of them 0;
    "holes" = every probe whose index is 1 mod 3 or 0 mod 5 has weight 0 and NaN coefficients, so that neighbouring points skip
    different corners; "zeros" = every weight 0"""
    rng = np.random.default_rng(seed + 17)
    sh = coefficients(g, seed)
    p = np.arange(g.probes)
    if mask == "ones":
        w = None
    elif mask == "fractional":
        w = rng.uniform(0.05, 2.0, size=g.probes).astype(F)
        w[rng.random(g.probes) < 0.25] = 0
    elif mask == "holes":
        w = np.ones(g.probes, dtype=F)
        off = (p % 3 == 1) | (p % 5 == 0)
        w[off] = 0
        sh[off] = np.nan
    elif mask == "zeros":
        w = np.zeros(g.probes, dtype=F)
    else:
        raise ValueError(mask)
    return V.pack(sh, w)


def uniform_points(g, n, seed=2):
    lo, hi = box(g)
    return np.random.default_rng(seed).uniform(lo, hi, size=(n, 3)).astype(F)


def normals(n, seed=3):
    """float32 (n, 3): unit, and every eighth zero, unnormalised (two kinds) or with a NaN component"""
    rng = np.random.default_rng(seed)
    d = Q._unit_sphere(rng, n)
    i = np.arange(n)
    d[i % 8 == 3] = 0
    d[i % 8 == 5] *= F(4.75)
    d[i % 8 == 6] *= F(0.125)
    d[i % 8 == 7, rng.integers(0, 3)] = np.nan
    return d


def points(g, n_uniform=2000, seed=2):
    """float32 (n, 6): positions uniform in the box, every probe position, points on cell faces, points far outside, points with
    infinite and NaN coordinates; normals as normals()"""
    rng = np.random.default_rng(seed + 5)
    lo, hi = box(g)
    pos = [uniform_points(g, n_uniform, seed), V.positions(g)]
    face = uniform_points(g, 3 * g.probes, seed + 1)
    pp = V.positions(g)
    for k in range(len(face)):  # one coordinate exactly on a probe plane
        face[k, k % 3] = pp[k // 3, k % 3]
    pos.append(face)
    span = np.maximum(hi - lo, 1.0)
    far = rng.uniform(lo - 3 * span, hi + 3 * span, size=(64, 3)).astype(F)
    far[::4] *= F(1e6)
    far[1::8] = far[1::8] * F(1e30)
    pos.append(far)
    odd = uniform_points(g, 48, seed + 2)
    for k in range(len(odd)):
        odd[k, k % 3] = (np.inf, -np.inf, np.nan)[(k // 3) % 3]
    odd[-1] = np.nan
    odd[-2] = (np.inf, -np.inf, np.inf)
    pos.append(odd)
    pos = np.concatenate(pos).astype(F)
    return np.concatenate([pos, normals(len(pos), seed + 3)], axis=1).astype(F)


def strided(pts, stride, fill=0xa5):
    """the (n, 6) points as n records of `stride` bytes, the bytes between them `fill`"""
    pts = np.ascontiguousarray(pts, dtype=F).reshape(-1, 6)
    buf = np.full((len(pts), stride), fill, dtype=np.uint8)
    buf[:, :24] = pts.view(np.uint8).reshape(len(pts), 24)
    return buf.reshape(-1)


def words(a):
    return Q._words(a)


@functools.lru_cache(maxsize=None)
def scene6(width=32):
    """(world, cam, rays float32 (n, 8), hits HIT_DTYPE (n,)) of scene 6: the feature pass's primary rays and the host form's hits"""
    world, cam = host.build_scene(6, width=width, spp=1)
    rays = Q.ray8(primary_rays(cam), Q.INF)
    hits = hip.query_closest_host(world, rays, nthreads=4)["hits"]
    assert (hits["flags"] & hip.HIT_HIT).mean() > 0.5
    return world, cam, rays, hits


def scene6_grid(count=(3, 3, 3)):
    """a grid inside the Cornell box"""
    return hip.VOLUME_GRID((100.0, 100.0, 100.0), (177.5, 177.5, 177.5), count, 0.5)

"""The reference side of the light-probe tests (tests/test_probe_host.py, tests/test_gpu_probe.py), from the oracle
and numpy alone.

mort_oracle_ray_color is called per (probe, direction, sample) as tests/radiance_ref.py calls it (its `0 +` sum); the rest of the
contract of include/mort_hip.h is restated here in numpy float32: the NaN guard, the nine basis expressions, the terms, the
x[0::2] + x[1::2] tree over a batch of 64, the batches in ascending order, the one scale.  The library's direction set is restated
in float64 from its formula.  reference() caches one answer per (world, directions, parameters) per process, and nothing may
change it."""
import functools
import math

import numpy as np

from mort_amd import hip
from tests import query_rays as Q
from tests import radiance_ref as R

F = np.float32
BATCH = 64
C0, C1, C2, C3, C4 = F(0.2820948), F(0.4886025), F(1.0925484), F(0.31539157), F(0.5462742)
TIMES = (0.0, 0.5, 1.0, 0.5, 1.0)


def fibonacci(D):
    """the spherical Fibonacci points in float64, rounded once: z = 1 - (2 j + 1) / D, r = sqrt(1 - z z), phi = j (pi (3 - sqrt 5))"""
    golden = math.pi * (3.0 - math.sqrt(5.0))
    out = np.zeros((D, 3), dtype=np.float64)
    for j in range(D):
        z = 1.0 - (2.0 * j + 1.0) / D
        r = math.sqrt(1.0 - z * z)
        phi = j * golden
        out[j] = (r * math.cos(phi), r * math.sin(phi), z)
    return out.astype(F)


def basis(dirs):
    """Y (D, 9) float32 at the directions as given, the contract's expressions"""
    d = np.asarray(dirs, dtype=F)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([np.full(len(d), C0, dtype=F), C1 * y, C1 * z, C1 * x, (C2 * x) * y, (C2 * y) * z,
                         C3 * ((F(3.0) * z) * z - F(1.0)), (C2 * x) * z, C4 * (x * x - y * y)], axis=1).astype(F)


def basis64(dirs):
    """the same expressions in float64 with the same constants: the quadrature bound's Y"""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = (float(c) for c in (C0, C1, C2, C3, C4))
    return np.stack([np.full(len(d), c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0), c2 * x * z,
                     c4 * (x * x - y * y)], axis=1)


def scale_of(D, samples):
    return F(4.0 * math.pi / float(D * samples))


def project(s, dirs, samples, order="contract"):
    """sh (n, 9, 3) from the direction sums s (n, D, 3).  order: "contract"; "descending" adds the batches from the last to the
    first; "sequential" sums a batch's terms one after the other -- the two the contract must be told from"""
    n, D = s.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(s != s, F(0), s).astype(F)
        term = (basis(dirs)[None, :, :, None] * g[:, :, None, :]).astype(F)  # (n, D, 9, 3)
        x = term.reshape(n, D // BATCH, BATCH, 27)
        if order == "sequential":
            acc = x[:, :, 0]
            for i in range(1, BATCH):
                acc = acc + x[:, :, i]
            x = acc
        else:
            for _ in range(6):
                x = x[:, :, 0::2] + x[:, :, 1::2]
            x = x[:, :, 0]
        batches = list(range(D // BATCH))
        if order == "descending":
            batches.reverse()
        acc = x[:, batches[0]]
        for b in batches[1:]:
            acc = acc + x[:, b]
        return (scale_of(D, samples) * acc).astype(F).reshape(n, 9, 3)


def probes_of(name, n=None):
    """PROBE_DTYPE records: the camera's lookfrom, the midpoint to lookat, the point 0.9 of the way, for a world with a unified tree
    one probe 100 x the reach outside the solids' box (it must take the scan), and a fifth at a quarter of the way; times 0, 0.5
    and 1 across them.  n: that many of them, the list repeated where it is shorter"""
    s = Q.build(name)
    a = np.array([s.cam.lookfrom.e[k] for k in range(3)], dtype=np.float64)
    b = np.array([s.cam.lookat.e[k] for k in range(3)], dtype=np.float64)
    pts = [a, a + 0.5 * (b - a), a + 0.9 * (b - a)]
    info = Q.reach(s.world)
    if info["tree"]:
        lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
        far = 0.5 * (lo + hi)
        far[0] = hi[0] + 100.0 * max(float(info["reach"]), 1.0)
        assert not Q.in_reach(info, far[None, :].astype(F))[0]
        pts.append(far)
    pts.append(a + 0.25 * (b - a))
    out = np.zeros(len(pts), dtype=hip.PROBE_DTYPE)
    out["position"] = np.array(pts).astype(F)
    out["time"] = TIMES[:len(pts)] if len(pts) == 5 else (0.0, 0.5, 1.0, 1.0)
    if n is not None:
        out = np.resize(out, n)
    return out


OWN_D = 64


def own_directions(kind):
    """a caller's set of 64: axis-parallel directions, two zero components, a zero-length entry, unnormalised entries; "nan":
    the same with one NaN direction"""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(OWN_D, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:6] = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    d[6] = (0, 0, 0)
    d[7:20] *= rng.uniform(0.01, 50.0, size=(13, 1))
    d = d.astype(F)
    if kind == "nan":
        d[33] = (np.nan, 0.5, 0.5)
    return d


def rays_of(probes, dirs):
    """(n D, 8): probe-major, the radiance query's rays"""
    n, D = len(probes), len(dirs)
    rays = np.zeros((n, D, 8), dtype=F)
    rays[:, :, 0:3] = probes["position"][:, None, :]
    rays[:, :, 3:6] = np.asarray(dirs, dtype=F)[None, :, :]
    rays[:, :, 6] = probes["time"][:, None]
    rays[:, :, 7] = np.inf
    return rays.reshape(n * D, 8)


class Ref:
    """probes (n,), dirs (D, 3), params, streams0 / streams (n D,), s (n, D, 3) the direction sums, sh (n, 9, 3)"""


@functools.lru_cache(maxsize=None)
def reference(name, D, samples=1, limit=None, n=None, dirs=None, background=None):
    """dirs: None = the library's set (restated), else a kind of own_directions"""
    s = Q.build(name)
    r = Ref()
    r.name, r.world = name, s.world
    r.cam = R.copy_camera(s.cam, limit, R.world_light(name), background)
    r.params = hip.probe_params_from_camera(r.cam, D, samples)
    r.probes = probes_of(name, n)
    r.dirs = fibonacci(D) if dirs is None else own_directions(dirs)
    assert len(r.dirs) == D
    nd = len(r.probes) * D
    r.streams0 = Q.some_streams(nd)
    r.streams = r.streams0.copy()
    r.s = R.oracle_radiance(s.world, r.cam, rays_of(r.probes, r.dirs), r.streams, samples).reshape(len(r.probes), D, 3)
    r.sh = project(r.s, r.dirs, samples)
    r.background = np.array([r.cam.background.e[k] for k in range(3)], dtype=F)
    for a in (r.probes, r.dirs, r.streams0, r.streams, r.s, r.sh):
        a.setflags(write=False)
    return r


def assert_equal(sh, streams, ref, what, n=None):
    """coefficients as raw words with any NaN equal to any NaN (Q._words), final streams as all 48 bytes; n: the first n probes"""
    D = len(ref.dirs)
    n = len(ref.probes) if n is None else n
    want = ref.sh[:n]
    sh = np.asarray(sh).reshape(-1, 9, 3)
    assert sh.shape == want.shape, what
    bad = np.argwhere(Q._words(sh) != Q._words(want))
    assert bad.size == 0, f"{what}: {len(bad)} coefficients differ, first probe {bad[0][0]} k {bad[0][1]} ch {bad[0][2]}: got {sh[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"
    a = np.asarray(streams).view(np.uint8).reshape(-1, 48)
    b = np.ascontiguousarray(ref.streams[:n * D]).view(np.uint8).reshape(-1, 48)
    assert a.shape == b.shape, what
    bad = np.flatnonzero((a != b).any(1))
    assert bad.size == 0, f"{what}: final stream differs for {bad.size} directions, first probe {bad[0] // D} direction {bad[0] % D}"


def census(name, limit=None):
    """The probes show something, asserted on the oracle's answers alone at D = 256.  Returns the figures."""
    r = reference(name, 256, 1, limit)
    with np.errstate(invalid="ignore"):
        plain = (r.s == r.background).all(2) | (r.s == 0).all(2)
        nan = np.isnan(r.s).any(2)
    coloured = (~plain & ~nan).mean(1)
    c0 = np.abs(r.sh[:, 0]).max(1)
    hi = np.abs(r.sh[:, 1:]).max((1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(c0 > 0, hi / c0, 0.0)
    out = dict(coloured=coloured, nan=nan.mean(1), ratio=ratio)
    assert ratio.max() >= 0.1, f"{name}: no probe has a coefficient of bands 1, 2 of a tenth of band 0: {ratio}"
    if name == "scene7":
        ok = (out["nan"] >= 0.10) & np.isfinite(r.sh).all((1, 2))
        assert ok.any(), f"{name}: no probe has 10 % NaN directions and finite coefficients: {out['nan']}"
    else:
        assert coloured.max() >= 0.10, f"{name}: no probe sees a colour other than the background or zero in 10 % of its directions: {coloured}"
    return out

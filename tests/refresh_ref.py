"""The reference side of the volume-refresh tests (tests/test_refresh_host.py, tests/test_gpu_refresh.py), made
from the oracle and numpy alone.

The selected probes' positions are restated from the grid, their rays built as the bake's (tests/probe_ref.rays_of) and walked by
tests/cached_ref.walk over the records the round reads; the guard, the terms and the sum order are tests/probe_ref.project; the
blend, the copy of a masked probe and the counts are restated here in numpy float32.  Worlds, grid, volumes and masks are
cached_ref's.  reference() caches one answer per case per process, and nothing may change it."""
import functools
import math

import numpy as np

import mort_amd.structs as S
from mort_amd import hip
from tests import cached_ref as CR
from tests import oracle_lib as O
from tests import probe_ref as PR
from tests import query_rays as Q
from tests import radiance_ref as R

F = np.float32
WORLDS = CR.WORLDS
MASKS = ("ones", "fractional", "holes", "slab", "poison")
SELECTIONS = ((0, 1, 24), (1, 5, 5), (23, 1, 1), (3, 7, 3))  # (first, step, m) on the P = 24 grid
LIMIT = 4
FILL = 0xa5


def positions(g):
    """PROBE_DTYPE (P,): origin[a] + (float)i_a * spacing[a], the product rounded, then the sum; index (iz ny + iy) nx + ix"""
    nx, ny, nz = g.count
    p = np.arange(g.probes)
    idx = (p % nx, (p // nx) % ny, p // (nx * ny))
    out = np.zeros(g.probes, dtype=hip.PROBE_DTYPE)
    for a in range(3):
        step = (idx[a].astype(F) * F(g.spacing[a])).astype(F)
        out["position"][:, a] = (F(g.origin[a]) + step).astype(F)
    out["time"] = F(g.time)
    return out


def selected(first, step, m):
    return first + step * np.arange(m)


def directions_round(D, r):
    """float64 restatement of mort_hip_probe_directions_round for r >= 1: the library's set rotated about direction r mod 64 of the
    64-point set by r golden angles (Rodrigues), rounded once"""
    golden = math.pi * (3.0 - math.sqrt(5.0))

    def fib(n):
        j = np.arange(n, dtype=np.float64)
        z = 1.0 - (2.0 * j + 1.0) / n
        rad = np.sqrt(1.0 - z * z)
        return np.stack([rad * np.cos(j * golden), rad * np.sin(j * golden), z], axis=1)
    v = fib(D)
    if r == 0:
        return v.astype(F)
    k = fib(64)[r % 64]
    th = r * golden
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = math.cos(th) * np.eye(3) + math.sin(th) * Kx + (1.0 - math.cos(th)) * np.outer(k, k)
    return (v @ Rm.T).astype(F)


def blend(old, new, h):
    """(h * old) + (om * new) with om = 1.0f - h; h == 0: new"""
    if F(h) == F(0):
        return new.astype(F)
    om = F(1.0) - F(h)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((F(h) * old).astype(F) + (om * new).astype(F)).astype(F)


def refresh(world, path, cache_depth, g, records_in, depth, vis, dirs, h, sel, streams, records_out, ends_out=None):
    """one call: streams (O.STATE_DTYPE, P D), records_out (P, 32) float32 and ends_out (P,) uint32 or None are written in place for
    the selected probes.  Returns the census: s (the active probes' direction sums, (n, D, 3)), active (their indices), the walk's"""
    first, step, m = sel
    D = len(dirs)
    P = g.probes
    assert streams.shape == (P * D,) and records_in.shape == (P, 32) and records_out.shape == (P, 32)
    probes = positions(g)
    sel_p = selected(first, step, m)
    assert m == 0 or sel_p[-1] < P
    with np.errstate(invalid="ignore"):
        live = records_in[sel_p, 27] > 0
    active, masked = sel_p[live], sel_p[~live]
    win, wout = records_in.view(np.uint32), records_out.view(np.uint32)
    wout[masked] = win[masked]
    if ends_out is not None:
        ends_out[masked] = 0
    cen = dict(active=active, masked=masked, s=np.zeros((0, D, 3), dtype=F), walk=None)
    if active.size == 0:
        return cen
    idx = (active[:, None] * D + np.arange(D)[None, :]).reshape(-1)
    sub = np.ascontiguousarray(streams[idx])
    rays = PR.rays_of(probes[active], dirs)
    rgb, ends, wc = CR.walk(world, path, cache_depth, g, records_in, depth, vis, rays, sub)
    streams[idx] = sub
    s = rgb.reshape(active.size, D, 3)
    new = PR.project(s, dirs, path.samples).reshape(active.size, 27)
    out = np.zeros((active.size, 32), dtype=F)
    out[:, :27] = blend(records_in[active, :27], new, h)
    ow = out.view(np.uint32)
    ow[:, 27] = win[active, 27]
    wout[active] = ow
    if ends_out is not None:
        ends_out[active] = ends.reshape(active.size, D).sum(1)
    cen.update(s=s, walk=wc, ends=ends.reshape(active.size, D))
    return cen


def path_of(name, samples=1, limit=LIMIT):
    s = Q.build(name)
    return hip.radiance_params_from_camera(R.copy_camera(s.cam, limit, R.world_light(name)), samples)


def streams_of(P, D):
    return O.seed_states(S.DEFAULT_SEED, P * D, 1)


def params_of(path, cache_depth, g, vis, D, h, sel):
    return hip.REFRESH_PARAMS(CR.params(path, cache_depth, g, vis), D, h, sel[0], sel[1])


class Ref:
    """world, grid, params (REFRESH_PARAMS), m, dirs, records_in, depth, streams0 / streams, records (P, 32; unselected FILL), ends
    (P,; unselected FILL words), census"""


@functools.lru_cache(maxsize=None)
def reference(name, cache_depth=0, h=0.0, samples=1, mask="ones", visible=False, D=64, sel=SELECTIONS[0], limit=LIMIT, dirs=None):
    """dirs: None = the library's set (restated), an int r = round r's set (restated), else a kind of PR.own_directions"""
    s = Q.build(name)
    g, rec, depth, vis = CR.volume(name, mask)
    r = Ref()
    r.name, r.world, r.grid = name, s.world, g
    r.path = path_of(name, samples, limit)
    r.dirs = PR.fibonacci(D) if dirs is None else directions_round(D, dirs) if isinstance(dirs, int) else PR.own_directions(dirs)
    assert len(r.dirs) == D
    r.records_in = rec
    r.depth, r.vis = (depth, vis) if visible else (None, None)
    r.sel, r.m = sel, sel[2]
    r.params = params_of(r.path, cache_depth, g, r.vis, D, h, sel)
    r.streams0 = streams_of(g.probes, D)
    r.streams = r.streams0.copy()
    r.records, r.ends = filled(g.probes)
    r.census = refresh(s.world, r.path, cache_depth, g, rec, r.depth, r.vis, r.dirs, h, sel, r.streams, r.records, r.ends)
    for a in (r.dirs, r.streams0, r.streams, r.records, r.ends):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def census_of_the_rays(name, cache_depth=0, mask="slab", visible=True, D=64):
    """the walk's census over the rays of EVERY probe of the grid, the masked ones included (the copy rule keeps those from running
    in a refresh): what the volume does to the grid's rays as such"""
    g, rec, depth, vis = CR.volume(name, mask)
    rays = PR.rays_of(positions(g), PR.fibonacci(D))
    return CR.walk(Q.build(name).world, path_of(name), cache_depth, g, rec, depth if visible else None, vis if visible else None, rays,
                   streams_of(g.probes, D))[2]


def filled(P, fill=FILL):
    """(records (P, 32) float32, ends (P,) uint32) of the fill byte"""
    return np.full(P * 128, fill, dtype=np.uint8).view(F).reshape(P, 32), np.full(P * 4, fill, dtype=np.uint8).view(np.uint32)


def assert_equal(records, streams, ends, ref, what):
    """records as raw words with any NaN equal to any NaN, all 48 bytes of every stream, the counts; the unselected records and
    counts against the fill they were given"""
    got, want = Q._words(np.asarray(records).reshape(-1, 32)), Q._words(ref.records)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} record words differ, first probe {bad[0][0]} float {bad[0][1]}: got {np.asarray(records).reshape(-1, 32)[tuple(bad[0])]!r} want {ref.records[tuple(bad[0])]!r}"
    a = np.asarray(streams).view(np.uint8).reshape(-1, 48)
    b = np.ascontiguousarray(ref.streams).view(np.uint8).reshape(-1, 48)
    assert a.shape == b.shape, what
    bad = np.flatnonzero((a != b).any(1))
    D = ref.params.directions
    assert bad.size == 0, f"{what}: final stream differs for {bad.size} directions, first probe {bad[0] // D} direction {bad[0] % D}"
    if ends is not None:
        bad = np.flatnonzero(np.asarray(ends) != ref.ends)
        assert bad.size == 0, f"{what}: counts differ for {bad.size} probes, first {bad[0]}: got {ends[bad[0]]} want {ref.ends[bad[0]]}"
